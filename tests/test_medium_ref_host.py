"""tests/medium_ref.py and tests/medium_edge_cases.py held to the oracle and to their own coverage conditions, without a GPU.

The oracle's list walk must be an element of the clamp set of every ray of every class: hit, t and the scattered origin bit for bit.  The
vectorised restatement is also held to the scalar composition of tests/golden/np_ref.py on a sample of every class.  Then the conditions that
keep tests/test_medium_edges.py from passing emptily, on the reference alone; the shares are printed class by class (pytest -s)."""
import numpy as np
import pytest

import medium_edge_cases as mc
import medium_ref as mr

f32 = np.float32


def _rows(bad):
    return int(bad.sum()), np.nonzero(bad)[0][:5]


@pytest.mark.parametrize("name", mc.CLASSES)
def test_the_oracles_list_walk_is_an_element_of_the_clamp_set(rt, orc, name):
    R = mc.reference(rt, orc, name)
    W = R["W"]
    for c in R["calls"]:
        got = orc.debug_bounce(R["scene"].flat_ptr, c["o"], c["d"], c["keys"], depth=c["depth"], accel=orc.ACCEL_LIST)
        S = c["clamp_ref"]
        e = mr.element(S, got["hit"], got["t"])
        assert (e >= 0).all(), (name, "outside the clamp set") + _rows(e < 0) + (got["hit"][e < 0][:5], got["t"][e < 0][:5], c["group"][e < 0][:5])
        med = got["hit"] >= W.n_prims
        p = S["p"][np.arange(len(e)), np.maximum(e, 0)]
        bad = med & (mr.bits(got["o"]) != mr.bits(p)).any(axis=1)
        assert not bad.any(), (name, "scattered origin") + _rows(bad) + (got["o"][bad][:3], p[bad][:3])
        assert got["alive"][med].all()
        bad = med & (mr.bits(got["d"]) != mr.bits(c["iso_d"])).any(axis=1)
        assert not bad.any(), (name, "the direction of an isotropic scatter") + _rows(bad)
        for m in range(W.n_media):  # a constant albedo is the attenuation, exactly
            col, _ = W.albedo(m)
            if col is not None:
                assert (mr.bits(got["attenuation"][got["hit"] == W.n_prims + m]) == mr.bits(col)).all(), (name, m)
        for k in ("t", "alive", "o", "d", "attenuation", "radiance"):  # a solid hit or a miss: the record of the scene without media
            assert np.array_equal(got[k][~med].view(np.uint8), c["solid"][k][~med].view(np.uint8)), (name, k)
        if name != "origins":  # the two conventions part only where a plane distance is NaN
            assert S is c["clamp"]
            for m in range(W.n_media):
                G = c["clamp"]["intervals"][m]
                assert not np.isnan(G["t1"][G["ok1"]]).any(), (name, m)
        else:
            apart = ~mr.same_sets(c["clamp_ref"], c["clamp"])
            print("origins: %d rays whose clamp set differs between the reference's NaN plane distance and the rejected one, groups %s"
                  % (apart.sum(), sorted(set(c["group"][apart]))))
            assert apart.any() and set(c["group"][apart]) <= {"face 0/0", "edge", "corner"}


@pytest.mark.parametrize("name", mc.CLASSES)
def test_the_vectorised_restatement_equals_the_scalar_one(rt, orc, name):
    """np_ref.constant_medium_hit over np_ref's sphere_hit / rect_hit / translate_hit / rotate_y_hit with the host's logarithm: its t is one of the
    set's, and where it reports no hit some admissible L does not either (120 rays of every medium's own targets)"""
    R = mc.reference(rt, orc, name)
    W = R["W"]
    rng = np.random.default_rng(3)
    for c in R["calls"][:1]:
        for m in range(W.n_media):
            own = np.nonzero(c["target"] == m)[0]
            idx = rng.choice(own if len(own) else np.arange(len(c["o"])), 120)
            ts = mr.medium_t_set(W, m, c["o"][idx], c["d"][idx], c["keys"][idx], c["depth"], nan_plane="reference")
            L, valid = mr.log_candidates(c["xi"][idx, m])
            for r, k in enumerate(idx):
                h = mr.scalar_medium(W, m, c["o"][k], c["d"][k], c["xi"][k, m], mr.FLT_MAX)
                if h is None:
                    assert np.isnan(ts[r][valid[r]]).any(), (name, m, k, ts[r])
                else:
                    assert (mr.bits(ts[r]) == mr.bits(h[0])).any() or (np.isnan(h[0]) and np.isnan(ts[r]).any()), (name, m, k, h[0], ts[r])


def test_the_draw_fixture_and_the_restated_draw(rt, orc):
    """every entry of tests/golden/medium_draw_keys.json gives its draw, through the oracle's exported generator too"""
    lib = orc.load()
    from helpers import path_keys
    for value, (depth, slot, m) in mc.DRAW_KEYS["draws"].items():
        key = path_keys(0, np.array([slot]), np.zeros(1, np.int64))
        xi = mr.medium_xi(key, depth, m)[0]
        assert xi == f32(int(value)) * f32(2.0 ** -24)
        assert lib.orc_ctr_draw(int(key[0, 0]), int(key[0, 1]), mr.medium_counter(depth, m)) >> 8 == int(value)
    assert mr.medium_counter(3, 31) == 1024 + 255 and mr.medium_counter(3, 32) == 0x40000000 + (1024 << 8) + 32
    R = mc.reference(rt, orc, "draws")
    seen = set()
    for c in R["calls"]:
        for k in np.nonzero(c["group"] != "spread")[0]:
            xi = c["xi"][k, c["target"][k]]
            seen.add(int(round(float(xi) * 2 ** 24)))
            G = c["winner"]["intervals"][c["target"][k]]
            assert G["ok"][k], "the chosen ray meets its medium"
            if xi == 0:  # -inf times a negative number: never scatters, under any rule
                assert not (c["clamp"]["hit"][k] == R["W"].n_prims + c["target"][k]).any() and not (c["winner"]["hit"][k] == R["W"].n_prims + c["target"][k]).any()
        spread = c["xi"][np.arange(len(c["o"])), c["target"]]
        assert len(np.unique((spread * 16).astype(int))) == 16
    assert seen == {0, 1, 2 ** 24 - 1}, seen


def _tie_distance(c):
    """of the rays whose clamp and winner sets differ: the smallest |t_medium - t_other| in ulp between a medium's outcome and another
    outcome of the ray (a wall, or another medium), i.e. how far apart the two candidates are where the rules part"""
    differ = ~mr.same_sets(c["clamp"], c["winner"])
    out = np.zeros(len(differ))
    for k in np.nonzero(differ)[0]:
        cand = {}
        for S in (c["clamp"], c["winner"]):
            for h, t in zip(S["hit"][k][S["valid"][k]], S["t"][k][S["valid"][k]]):
                cand.setdefault(int(h), set()).add(int(mr.bits(f32(t)).reshape(-1)[0]))
        if c["solid"]["hit"][k] >= 0:
            cand.setdefault(int(c["solid"]["hit"][k]), set()).add(int(mr.bits(c["solid"]["t"][k]).reshape(-1)[0]))
        hits = sorted(cand)
        best = min((abs(a - b) for i, h in enumerate(hits) for g in hits[i + 1:] for a in cand[h] for b in cand[g]), default=0)
        out[k] = best
    return differ, out


@pytest.mark.parametrize("name", mc.CLASSES)
def test_every_class_meets_its_coverage_conditions(rt, orc, name):
    R = mc.reference(rt, orc, name)
    W = R["W"]
    n = sum(len(c["o"]) for c in R["calls"])
    sh = {k: np.concatenate([mc.shares(c)[k] for c in R["calls"]]) for k in ("multi", "differ", "scatters", "passes")}
    sizes = np.concatenate([np.maximum(c["clamp"]["valid"].sum(axis=1), c["winner"]["valid"].sum(axis=1)) for c in R["calls"]])
    print("%s: %d rays, %d media; more than one hit index %.4f, clamp and winner sets differ %.4f, always scatter %.3f, never scatter %.3f, largest set %d"
          % (name, n, W.n_media, sh["multi"].mean(), sh["differ"].mean(), sh["scatters"].mean(), sh["passes"].mean(), sizes.max()))
    assert n <= 4096
    if name == "ties":
        worst = 0
        for c in R["calls"]:
            differ, dist = _tie_distance(c)
            worst = max(worst, int(dist[differ].max(initial=0)))
            for g in sorted(set(c["group"])):
                sel = c["group"] == g
                print("  ties, %s: %d rays, %d multi, %d with clamp != winner, largest distance where they part %d ulp"
                      % (g, sel.sum(), sh["multi"][sel].sum(), differ[sel].sum(), dist[sel & differ].max(initial=0)))
            tuned = c["aim"][np.isin(c["group"], ("wall at the scatter point", "two media at one point"))]
            assert set(tuned) == set(range(-3, 4))
        assert (sh["multi"] | sh["differ"]).mean() >= 0.5, (sh["multi"] | sh["differ"]).mean()
        print("  ties: the largest |t_medium - t_other| at which the clamp and the winner rule part: %d ulp" % worst)
        assert {"floor at the exit", "floor at the entry", "floor at the entry, dense", "floor at the exit, dense"} <= set(R["calls"][0]["group"])
    else:
        assert sh["multi"].mean() <= 1e-3
    assert sh["scatters"].mean() >= 0.10 and sh["passes"].mean() >= 0.10
    c = R["calls"][0]
    G = c["winner"]["intervals"]
    own = lambda key: np.array([G[m][key][k] for k, m in enumerate(c["target"])])
    if name == "densities":
        for k, dens in enumerate(mc.DENSITIES):
            for m in (2 * k, 2 * k + 1):  # (the host mirror halves it for a medium that a BvhNode holds as both children, hitable.rs:188)
                assert np.isclose(W.neg_inv_density[m], -1.0 / dens, rtol=1e-6) or np.isclose(W.neg_inv_density[m], -0.5 / dens, rtol=1e-6)
        t1, tm = own("t1"), c["winner"]["t"][:, 0]
        dense = (c["target"] >= 8) & (c["winner"]["hit"][:, 0] == W.n_prims + c["target"]) & (t1 > 0)
        assert dense.sum() > 200 and (np.abs(mc._ulps(tm[dense], t1[dense].astype(f32))) <= 16).mean() > 0.9  # within a few ulp of the entry
        thin = c["target"] < 2
        assert (c["winner"]["hit"][thin, 0] == W.n_prims + c["target"][thin]).mean() < 0.01                # almost never
    if name == "window":
        t2, tmin2, ok1, ok = own("t2"), own("t_min2"), own("ok1"), own("ok")
        for g in sorted(set(c["group"])):
            sel = (c["group"] == g) & ok1
            found, lost = (sel & ok).sum(), (sel & ~ok).sum()
            near = (sel & ok & (np.abs(mc._ulps(t2, tmin2)) <= 2)).sum()
            print("  window, %s: %d rays meet the boundary, second search finds a root %d, none %d, a root within 2 ulp of t1 + 0.0001: %d" % (g, sel.sum(), found, lost, near))
            assert found >= 0.1 * sel.sum() and lost >= 0.1 * sel.sum() and (near >= 3 or g.startswith("tangent")), g
        with np.errstate(all="ignore"):
            for m, tag in ((4, "tangent |d|=1"), (5, "tangent |d|=1000")):
                a, i = W.a, int(W.boundary[m][0])
                sel = c["group"] == tag
                _, _, disc = mr._sphere_t((a["sph_cx"][i], a["sph_cy"][i], a["sph_cz"][i]), a["sph_r"][i], mr._cols(c["o"][sel]), mr._cols(c["d"][sel]), -mr.INF, mr.INF)
                tiny = (disc > 0) & (own("t2")[sel] - own("t1")[sel] < 2e-4)
                print("  window, %s: discriminant negative %d, zero %d, positive %d (t2 - t1 below 2e-4: %d)" % (tag, (disc < 0).sum(), (disc == 0).sum(), (disc > 0).sum(), tiny.sum()))
                assert (disc < 0).sum() >= 10 and (disc == 0).sum() >= 1 and tiny.sum() >= 10
    if name == "far_entry":
        t1 = own("t1")
        for g in ("outside", "inside"):
            a = np.abs(t1[(c["group"] == g) & own("ok1")])
            sign = t1[(c["group"] == g) & own("ok1")]
            assert (sign > 0).all() if g == "outside" else (sign < 0).all()
            counts = [(a < 1024).sum(), ((a >= 1024) & (a < 2048)).sum(), (a >= 2048).sum()]
            print("  far_entry, %s: |t1| below 1024: %d, 1024 .. 2048: %d, from 2048: %d" % (g, *counts))
            assert min(counts) >= 100
        far = np.abs(t1) >= 2048  # the second search finds the first root again: the target never scatters
        assert not (c["winner"]["hit"][far] == (W.n_prims + c["target"][far])[:, None]).any()
        mist_centre = (c["target"] == 0) & (np.abs(t1) >= 2048)
        assert mist_centre.sum() >= 100
    if name == "origins":
        assert set(c["group"]) == {"inside", "face 0/0", "edge", "corner", "sphere surface", "looking away"}
        face = c["group"] == "face 0/0"
        Gr = W.interval(0, c["o"][face], c["d"][face], "reference")
        assert np.isnan(Gr["t1"]).mean() > 0.9
        away = c["group"] == "looking away"
        assert (own("t2")[away & own("ok")] < mr.T_MIN).all() and (away & own("ok")).sum() > 50


def test_every_wrapped_form_is_the_form_it_says(rt, orc):
    """from the flat arrays alone: which chain the boundary shares, which wrapper stands around the medium, how many rectangles bound it"""
    for name in mc.CLASSES:
        if not name.startswith("wrapped_"):
            continue
        W = mc.reference(rt, orc, name)["W"]
        form = name[8:]
        for m in range(W.n_media):
            chains = {W.prim_xform(int(i)) for i in W.boundary[m]}
            below = [len(mr._chain(W.a, x, W.med_xform[m])) for x in chains]
            if form == "common":
                assert W.med_xform[m] == mr.NONE and len(chains) == 1 and below == [2]
            elif form == "around":
                assert W.med_xform[m] != mr.NONE and below == [0] and len(mr._chain(W.a, W.med_xform[m])) == 2
            elif form == "both":
                assert W.med_xform[m] != mr.NONE and below == [2] and len(mr._chain(W.a, W.med_xform[m])) == 2
            elif m == 1:
                assert len(W.boundary[m]) == 12 and len(chains) == (1 if form == "slow" else 2)
