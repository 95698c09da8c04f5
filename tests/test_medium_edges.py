"""ConstantMedium::hit on the GPU at its edges, held to the set-valued reference of tests/medium_ref.py (the same scenes and rays as
tests/test_medium_ref_host.py, which holds the reference to the oracle and the classes to their coverage conditions).

Every class of tests/medium_edge_cases.py goes through rt_debug_bounce in its default form (the tree), with FLAG_BRUTE_FORCE (the list walk),
with FLAG_PRODUCTION_KERNELS and with both, with the tree in LDS and behind L2, the wrapper / medium tables in LDS and in memory, and with
the boundary searched once (medium_search 0) and twice (1).  A list-walk path must return an element of the ray's CLAMP set, a tree path
an element of its WINNER set: hit, t, alive and the scattered origin bit for bit against that element, the direction of a medium's scatter
the isotropic draw bit for bit, a constant albedo exactly and a textured one to the colour tolerance at that element's p.  A solid hit or a
miss is the record of the scene without its media.  Every setting must give the bytes of the first one, and where a ray's two sets are the
same single outcome all four paths agree bit for bit."""
import numpy as np
import pytest

import medium_edge_cases as mc
import medium_ref as mr
from frame_replay import near_one
from helpers import primary_rays

pytestmark = pytest.mark.gpu
f32 = np.float32
SETTINGS = [("tree in LDS", {}), ("tree behind L2", {"tree_placement": 1}), ("tables in memory", {"general_lds": 1}), ("two searches", {"medium_search": 1}),
            ("tree behind L2, tables in memory, two searches", {"tree_placement": 1, "general_lds": 1, "medium_search": 1})]
FIELDS = ("hit", "t", "alive", "o", "d", "attenuation", "radiance")


def _paths(rt):
    f = rt._ffi
    return [("tree", 0), ("list walk", f.FLAG_BRUTE_FORCE), ("production", f.FLAG_PRODUCTION_KERNELS), ("production list walk", f.FLAG_PRODUCTION_KERNELS | f.FLAG_BRUTE_FORCE)]


def _rows(bad):
    return int(bad.sum()), np.nonzero(bad)[0][:5]


def _dropped(c, production):
    """the production kernels shade only rays whose direction is of unit length to a few ulp (k_shade drops the others: frame_replay.near_one);
    their closest hit is reported all the same"""
    return ~near_one(c["d"]) if production else np.zeros(len(c["d"]), bool)


def _check(orc, R, c, got, rule, what, production):
    """one call's result against the sets of `rule`"""
    W, S, solid = R["W"], c[rule], c["solid"]
    e = mr.element(S, got["hit"], got["t"])
    bad = e < 0
    assert not bad.any(), (what, "outside the %s set" % rule) + _rows(bad) + (got["hit"][bad][:5], got["t"][bad][:5], c["group"][bad][:5], S["hit"][bad][:5], S["t"][bad][:5])
    drop = _dropped(c, production)
    assert not got["alive"][drop].any() and (~drop).sum() >= 500, (what, "rays the production kernels drop")
    got = {k: v[~drop] for k, v in got.items()}
    c = dict(c, group=c["group"][~drop], iso_d=c["iso_d"][~drop])
    solid = {k: v[~drop] for k, v in solid.items()}
    e, S = e[~drop], dict(S, p=S["p"][~drop])
    med = got["hit"] >= W.n_prims
    p = S["p"][np.arange(len(e)), e]
    assert got["alive"][med].all(), (what, "a medium's scatter lives")
    bad = med & (mr.bits(got["o"]) != mr.bits(p)).any(axis=1)
    assert not bad.any(), (what, "scattered origin") + _rows(bad) + (got["o"][bad][:3], p[bad][:3], c["group"][bad][:5])
    bad = med & (mr.bits(got["d"]) != mr.bits(c["iso_d"])).any(axis=1)
    assert not bad.any(), (what, "isotropic direction") + _rows(bad)
    assert not got["radiance"][med].any(), what
    for m in range(W.n_media):
        of = got["hit"] == W.n_prims + m
        col, tex = W.albedo(m)
        if col is not None:
            assert (mr.bits(got["attenuation"][of]) == mr.bits(col)).all(), (what, "constant albedo", m)
        elif of.any():
            want = mc.texture_colour(orc, R["scene"], tex, p[of])
            assert np.allclose(got["attenuation"][of], want, rtol=2e-5, atol=1e-6), (what, "textured albedo", m, np.abs(got["attenuation"][of] - want).max())
    rest = ~med  # (hit and t are the element's: the closest solid primitive or a miss)
    assert np.array_equal(got["alive"][rest], solid["alive"][rest]), (what, "alive of a solid hit")
    live = rest & (solid["alive"] == 1)
    for k in ("o", "d"):
        assert np.array_equal(mr.bits(got[k][live]), mr.bits(solid[k][live])), (what, k, "of a solid hit")
    assert np.allclose(got["attenuation"][live], solid["attenuation"][live], rtol=2e-5, atol=1e-6), what
    assert np.allclose(got["radiance"][rest & ~live], solid["radiance"][rest & ~live], rtol=2e-5, atol=1e-6), what


def _expected_info(name, setting):
    nest = 1 if name in ("wrapped_around", "wrapped_both") else 0
    return dict(tree_in_lds=0 if setting.get("tree_placement") else 1, general_tables_in_lds=0 if setting.get("general_lds") else 1, nest=nest, general_kernels=1)


@pytest.mark.parametrize("name", mc.CLASSES)
def test_every_path_returns_an_element_of_its_set(rt, orc, renderer, name):
    R = mc.reference(rt, orc, name)
    first = {}
    for label, setting in SETTINGS:
        for k, v in setting.items():
            renderer.set_option(k, v)
        try:
            renderer.upload(mc.uploadable(rt, R["scene"]))
        finally:
            for k in setting:
                renderer.set_option(k, 0)
        info = renderer.scene_info()
        want = _expected_info(name, setting)
        assert {k: info[k] for k in want} == want, (name, label, info)
        for ci, c in enumerate(R["calls"]):
            for path, flags in _paths(rt):
                what = (name, label, path, "call %d" % ci)
                got = renderer.debug_bounce(c["o"], c["d"], c["keys"], depth=c["depth"], flags=flags)
                if (ci, path) not in first:
                    _check(orc, R, c, got, "clamp" if "list walk" in path else "winner", what, "production" in path)
                    first[(ci, path)] = got
                else:  # every placement, and one boundary evaluation or two: the same bytes on every ray
                    for k in FIELDS:
                        bad = (got[k].view(np.uint8).reshape(len(got[k]), -1) != first[(ci, path)][k].view(np.uint8).reshape(len(got[k]), -1)).any(axis=1)
                        assert not bad.any(), (what, k, "differs from the first setting") + _rows(bad) + (c["group"][bad][:5],)
    for ci, c in enumerate(R["calls"]):  # one outcome under both rules: all four paths agree
        one = (c["clamp"]["valid"].sum(axis=1) == 1) & (c["winner"]["valid"].sum(axis=1) == 1) & mr.same_sets(c["clamp"], c["winner"])
        assert one.mean() > (0.2 if name == "ties" else 0.4), (name, one.mean())  # (ties: most of its sets hold several outcomes)
        tree = first[(ci, "tree")]
        for path, _ in _paths(rt)[1:]:
            for k in ("hit", "t", "alive", "o", "d"):
                sel = one if k in ("hit", "t") else one & ~_dropped(c, "production" in path)
                assert np.array_equal(first[(ci, path)][k][sel].view(np.uint8), tree[k][sel].view(np.uint8)), (name, path, k)
            live = one & (tree["alive"] == 1) & ~_dropped(c, "production" in path)
            assert np.array_equal(first[(ci, path)]["attenuation"][live].view(np.uint8), tree["attenuation"][live].view(np.uint8)), (name, path, "attenuation")


def _trace(renderer, scene, p, ii, jj, ss, flags):
    """the paths (pixel column ii, row jj, sample ss) bounce by bounce through rt_debug_bounce(flags), the estimator of k_shade restated as in
    tests/frame_replay.py -> (value [n, 3], rays: per depth dict(path, o, d, keys, out))"""
    import frame_replay as fr
    o, d, keys = primary_rays(scene, p, ii, jj, ss)
    n = len(ii)
    value, T, path, rays = np.zeros((n, 3), f32), np.ones((n, 3), f32), np.arange(n), []
    for depth in range(int(p.max_depth) + 1):
        ok = fr.near_one(d)
        path, o, d, T = path[ok], o[ok], d[ok], T[ok]
        if len(path) == 0:
            break
        out = renderer.debug_bounce(o, d, keys[path], depth=depth, flags=flags)
        rays.append(dict(path=path, o=o, d=d, keys=keys[path], out=out))
        live = out["alive"] == 1
        value[path[~live]] = (T[~live] * out["radiance"][~live]).astype(f32)
        if depth == int(p.max_depth):
            break
        path, o, d, T = path[live], out["o"][live], out["d"][live], (T[live] * out["attenuation"][live]).astype(f32)
    return value, rays


def test_a_frame_differs_between_tree_and_list_walk_only_where_the_rules_do(rt, orc, renderer):
    """32 x 32 pixels, 4 spp, depth 8 of the `ties` scene, seen from below the floor its dense box stands on: the tree and FLAG_BRUTE_FORCE.
    Every pixel that differs is re-traced path by path through both single-kernel hooks; each of its paths that parts does so at a ray whose
    clamp and winner sets differ, both pixels are the in-order sums of their own paths, and a pixel without such a ray may not differ."""
    import frame_replay as fr
    R = mc.reference(rt, orc, "ties")
    scene, W = R["scene"], R["W"]
    renderer.upload(scene)
    p = rt.make_params(32, 32, 4, max_depth=8, seed=7)
    tree = renderer.render(scene.camera, p)[0]
    walk = renderer.render(scene.camera, rt.make_params(32, 32, 4, max_depth=8, seed=7, flags=rt._ffi.FLAG_BRUTE_FORCE))[0]
    jj, ii = np.nonzero((tree.view(np.uint32) != walk.view(np.uint32)).any(axis=2))
    print("ties frame: %d of 1024 pixels differ between the tree and the list walk" % len(ii))
    assert len(ii) >= 8, "the frame does not reach the floor below the dense box"
    i4, j4, s4 = np.repeat(ii, 4), np.repeat(jj, 4), np.tile(np.arange(4), len(ii))
    va, ra = _trace(renderer, scene, p, i4, j4, s4, 0)
    vb, rb = _trace(renderer, scene, p, i4, j4, s4, rt._ffi.FLAG_BRUTE_FORCE)
    for v, img, what in ((va, tree, "tree"), (vb, walk, "list walk")):  # each image is the sum of its own hook's paths
        pix = fr.mean_in_order(v.reshape(len(ii), 4, 1, 3).transpose(1, 0, 2, 3))[:, 0]
        assert np.array_equal(pix.view(np.uint32), img[jj, ii].view(np.uint32)), what
    parted = np.zeros(len(i4), bool)
    n_rays = 0
    for depth, (a, b) in enumerate(zip(ra, rb)):
        both = np.isin(a["path"], b["path"]) & ~parted[a["path"]]
        ka = np.nonzero(both)[0]
        kb = np.searchsorted(b["path"], a["path"][ka])
        assert np.array_equal(b["path"][kb], a["path"][ka])
        same_ray = (mr.bits(a["o"][ka]) == mr.bits(b["o"][kb])).all(axis=1) & (mr.bits(a["d"][ka]) == mr.bits(b["d"][kb])).all(axis=1)
        assert same_ray.all(), "paths that have not parted trace the same ray"
        differ = np.zeros(len(ka), bool)
        for k in ("hit", "t", "alive", "o", "d", "attenuation", "radiance"):
            x, y = a["out"][k][ka], b["out"][k][kb]
            differ |= (x.view(np.uint8).reshape(len(ka), -1) != y.view(np.uint8).reshape(len(ka), -1)).any(axis=1)
        if differ.any():
            o, d, keys = a["o"][ka][differ], a["d"][ka][differ], a["keys"][ka][differ]
            s = orc.debug_bounce(R["twin"].flat_ptr, o, d, keys, depth=depth, accel=orc.ACCEL_LIST)
            sh = np.where(s["hit"] >= 0, W.solid_ids[np.maximum(s["hit"], 0)], -1).astype(np.int32)
            sets = [mr.outcomes(W, o, d, keys, depth, sh, s["t"], rule) for rule in ("clamp", "winner")]
            assert not mr.same_sets(*sets).any(), ("a ray on which tree and list walk differ although its clamp and winner sets are the same", depth, o[:3], d[:3])
            for hook, S, out, kk in (("tree", sets[1], a["out"], ka), ("list walk", sets[0], b["out"], kb)):
                assert (mr.element(S, out["hit"][kk][differ], out["t"][kk][differ]) >= 0).all(), (hook, depth)
            parted[a["path"][ka][differ]] = True
            n_rays += int(differ.sum())
    print("ties frame: %d paths part, each at a ray whose clamp and winner sets differ" % n_rays)
    assert parted.reshape(len(ii), 4).any(axis=1).all(), "a pixel differs although none of its paths parts"
