"""Culling of primitives below Translate / RotateY chains, held against the reference's wrapper semantics in float64.

The closest-hit searches (list walk, tree in LDS or through L2, per-pixel candidate lists, production kernels) must return the same
bits except on rays that fp32 reports as a hit although they miss in exact arithmetic (include/rtow_mi355x_debug.h).  For a wrapped
primitive "exact" means the chain's own ray map taken without rounding (tests/exact_wrappers.py): so every bound the searches cull
with must contain the exact world region of the primitive, and a ray the exact map puts inside a primitive by more than fp32 can
move it must be hit by every search.

The CPU tests read the bounds through rt_debug_world_bounds (the function rt_scene_upload builds the tree and the candidate-list
spheres from); the GPU tests aim rays at silhouettes and edges through the exact map and compare the searches."""
import ctypes as C

import numpy as np
import pytest

import exact_wrappers as ew
from helpers import path_keys, primary_rays

# RotateY angles whose stored f32 (sin, cos) are furthest from the unit circle, of either sign (checked below), and final_scene's 15
ANGLE_S2_ABOVE, ANGLE_S2_BELOW = 132.0, 138.4  # (of the angles in steps of 0.1 degree)
KINDS = ["rot_above", "rot_below", "rot15", "cancel1e2", "cancel1e4", "cancel1e6", "pivot", "mix"]
DEPTHS = [1, 2, 4, 5, 18, 64, 128, 256]
PIVOT = (700.0, 0.0, -450.0)


def _wrappers(kind, depth):
    """The chain of `kind` with `depth` wrappers, innermost first: ("t", offset) or ("r", degrees)."""
    out = []
    k = 0
    while len(out) < depth:
        if kind == "rot_above":
            out.append(("r", ANGLE_S2_ABOVE))
        elif kind == "rot_below":
            out.append(("r", ANGLE_S2_BELOW))
        elif kind == "rot15":
            out.append(("r", 15.0))
        elif kind.startswith("cancel"):
            m = float(kind[len("cancel"):])
            sgn = 1.0 if k % 2 == 0 else -1.0
            out.append(("t", (sgn * m, sgn * m * 0.37, -sgn * m * 0.61)))
        elif kind == "pivot":  # rotate about a far pivot: Translate(P) . RotateY . Translate(-P)
            out += [("t", tuple(-x for x in PIVOT)), ("r", (15.0, ANGLE_S2_ABOVE, ANGLE_S2_BELOW)[k % 3]), ("t", PIVOT)]
        else:  # mixtures of all of the above
            step = k % 6
            if step == 0:
                out += [("t", (1e4, 0.0, -1e4)), ("r", ANGLE_S2_ABOVE), ("t", (-1e4, 0.0, 1e4))]
            elif step == 1:
                out.append(("r", ANGLE_S2_BELOW))
            elif step == 2:
                out += [("t", (1e6, 3.0, 0.0)), ("t", (-1e6, -3.0, 0.0))]
            elif step == 3:
                out += [("t", tuple(-x for x in PIVOT)), ("r", 15.0), ("t", PIVOT)]
            elif step == 4:
                out.append(("t", (0.25, -0.5, 1e2)))
            else:
                out.append(("r", ANGLE_S2_ABOVE))
        k += 1
    return out[:depth]


def _wrap(s, h, kind, depth):
    for w, v in _wrappers(kind, depth):
        h = s.translate(h, v) if w == "t" else s.rotate_y(h, v)
    return h


def wrapped_scene(rt, kind, depth):
    """A sphere, rectangles on all three axes (edges at 0.55 as in the cancelling-translate case), a GBox, a medium in a sphere and a
    medium in a box with the wrappers around the medium, each below its own chain of `kind`; nothing is bare."""
    f = rt._ffi
    s = rt.Scene.new()
    white = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.73, 0.73, 0.73)))
    light = s.material(f.MAT_EMISSION, tex0=s.constant_tex((4.0, 4.0, 4.0)))
    fog = s.constant_tex((0.8, 0.8, 0.9))
    _wrap(s, s.sphere((0.3, 0.2, -0.1), 0.5, white, "ball"), kind, depth)
    _wrap(s, s.rect(f.RECT_XZ, (-0.45, -0.9, -0.45), (0.55, -0.9, 0.55), light), kind, depth)
    _wrap(s, s.rect(f.RECT_XY, (-0.45, -0.45, 1.2), (0.55, 0.55, 1.2), white), kind, depth)
    _wrap(s, s.rect(f.RECT_YZ, (-1.3, -0.45, -0.45), (-1.3, 0.55, 0.55), white), kind, depth)
    _wrap(s, s.gbox((1.0, -0.5, -0.5), (1.55, 0.55, 0.25), white), kind, depth)
    s.constant_medium(_wrap(s, s.sphere((-0.2, 1.3, 0.4), 0.35, white, "boundary"), kind, depth), 2.0, fog)
    _wrap(s, s.constant_medium(s.gbox((0.6, 1.0, 0.5), (1.1, 1.55, 1.05), white), 2.0, fog), kind, depth)
    return s


def _finished(rt, kind, depth, eye=(0.5, 0.5, 6.0), target=(0.5, 0.3, 0.0), vfov=40.0):
    s = wrapped_scene(rt, kind, depth)
    s.set_camera(eye, target, (0, 1, 0), vfov, 1.0)
    return s.finish()


def _inside_box(lo, hi, blo, bhi):
    """How far (>= 0: inside) the box [lo, hi] lies within [blo, bhi], per box: the smallest of the six gaps."""
    return min(float(np.min(np.asarray(lo) - np.asarray(blo, np.float64))), float(np.min(np.asarray(bhi, np.float64) - np.asarray(hi))))


def _inside_ball(points, centre, radius):
    return float(radius) - float(np.linalg.norm(np.asarray(points, np.float64).reshape(-1, 3) - np.asarray(centre, np.float64), axis=1).max())


def _bound_margins(rt, scene):
    """Per primitive, the worst (smallest) margin by which every bound culling uses contains its exact world region, in units of the
    primitive's size: padded tree box, world sphere (spheres), the entry's tree box and candidate-list sphere (a medium's: for each
    boundary primitive).  Negative = part of the exact region lies outside."""
    fs = scene.flat
    wb = rt.world_bounds(scene)
    prims = ew.primitives(fs)
    entry_of = {int(e): k for k, e in enumerate(wb["entry_id"])}
    n_prims = fs.n_spheres + fs.n_rects
    out = []
    for p in prims:
        lo, hi = p.world_box()
        m = [_inside_box(lo, hi, wb["prim_box_padded"][p.id][0], wb["prim_box_padded"][p.id][1])]
        c, r = p.world_ball()
        if p.sphere:
            ws = wb["world_sphere"][p.id]
            m.append(float(ws[3]) - (np.linalg.norm(c - ws[:3].astype(np.float64)) + r))
        med = fs.sph_medium[p.id] if p.sphere else fs.rect_medium[p.id - fs.n_spheres]
        e = entry_of[p.id if med == ew.NO_XFORM else n_prims + int(med)]
        m.append(_inside_box(lo, hi, wb["entry_box_padded"][e][0], wb["entry_box_padded"][e][1]))
        bs = wb["entry_bs"][e]
        pts = np.array([c + r * u for u in np.eye(3)] + [c - r * u for u in np.eye(3)]) if p.sphere else ew.object_to_world(p.ch, p.corners())
        if p.sphere:
            m.append(float(bs[3]) - (np.linalg.norm(c - bs[:3].astype(np.float64)) + r))
        else:
            m.append(_inside_ball(pts, bs[:3], bs[3]))
        out.append(min(m) / p.size)
    return np.array(out), prims


def test_rotate_y_angles_are_the_extremes_of_the_stored_sin_cos(rt):
    """Of the angles 0.1 ... 179.9 degrees in steps of 0.1, the two chosen give the largest sin^2 + cos^2 - 1 of the stored f32 pair
    above and below 1 (one ulp of it near 1 is 6e-8)."""
    s = rt.Scene.new()
    white = s.material(rt._ffi.MAT_DIFFUSE, tex0=s.constant_tex((0.5, 0.5, 0.5)))
    angles = [k / 10 for k in range(1, 1800)]
    for a in angles:
        s.rotate_y(s.sphere((0, 0, 0), 1.0, white, "s"), a)
    s.set_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40, 1.0)
    s.finish()
    d = np.array([ew.s2_minus_1(x) for x in s.arrays()["xf_param"].reshape(-1, 4)])
    assert angles[int(np.argmax(d))] == ANGLE_S2_ABOVE and angles[int(np.argmin(d))] == ANGLE_S2_BELOW, (d.max(), d.min())
    assert d.max() > 7.5e-8 and d.min() < -7.5e-8


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_culling_bounds_contain_the_exact_world_region(rt, kind, depth):
    scene = _finished(rt, kind, depth)
    m, prims = _bound_margins(rt, scene)
    worst = int(np.argmin(m))
    print(f"{kind} depth {depth}: worst bound margin {m[worst]:+.3e} of the primitive's size (primitive {worst}, "
          f"{'sphere' if prims[worst].sphere else 'rectangle'})")
    assert (m >= 0).all(), [(i, float(m[i])) for i in np.flatnonzero(m < 0)]


def test_cancelling_translates_keep_the_rectangle_edge(rt):
    """The issue's own example: an edge at x = 0.55 below Translate(+1e4) inside Translate(-1e4) is where it was."""
    f = rt._ffi
    s = rt.Scene.new()
    white = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.73, 0.73, 0.73)))
    s.translate(s.translate(s.rect(f.RECT_XZ, (-0.45, 0.0, -0.45), (0.55, 0.0, 0.55), white), (1e4, 0.0, 0.0)), (-1e4, 0.0, 0.0))
    s.set_camera((0, 2, 5), (0, 0, 0), (0, 1, 0), 40, 1.0)
    s.finish()
    wb = rt.world_bounds(s)
    assert wb["prim_box_padded"][0][1][0] >= 0.55 and wb["prim_box_padded"][0][0][0] <= -0.45, wb["prim_box_padded"][0]


@pytest.mark.parametrize("name", ["sphere_scene", "cornell_box", "final_scene", "test_sphere", "earth_env_scene", "pbr_sweep_scene"])
def test_demo_scene_bounds_contain_the_exact_world_region(rt, name):
    scene = rt.Scene.build(name, 1.0)
    if not scene.flat.n_xforms:
        assert rt.world_bounds(scene)["prim_box"].shape[0] == scene.flat.n_spheres + scene.flat.n_rects
        return
    m, _ = _bound_margins(rt, scene)
    print(f"{name}: worst bound margin {m.min():+.3e}")
    assert (m >= 0).all()


def test_world_bounds_hook_refuses_bad_scenes(rt):
    f = rt._ffi
    s = rt.Scene.new()
    white = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.5, 0.5, 0.5)))
    s.translate(s.sphere((0, 0, 0), 1.0, white, "s"), (1.0, 2.0, 3.0))
    s.set_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40, 1.0)
    s.finish()
    fs = f.RtFlatScene.from_buffer_copy(s.flat)
    par = (C.c_uint32 * 1)(5)  # a parent that does not precede its child
    fs.xf_parent = C.cast(par, C.POINTER(C.c_uint32))
    with pytest.raises(rt.RtError):
        rt.world_bounds(fs)
    m = rt.Scene.new()
    white = m.material(f.MAT_DIFFUSE, tex0=m.constant_tex((0.5, 0.5, 0.5)))
    m.constant_medium(m.sphere((0, 0, 0), 1.0, white, "b"), 1.0, m.constant_tex((0.5, 0.5, 0.5)))
    m.set_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40, 1.0)
    m.finish()
    assert len(rt.world_bounds(m)["entry_id"]) == 1
    fm = f.RtFlatScene.from_buffer_copy(m.flat)
    fm.n_media = 2  # a second medium that no primitive bounds (rt_scene_upload refuses it)
    with pytest.raises(rt.RtError):
        rt.world_bounds(fm)
    wb = rt.world_bounds(s)
    assert np.allclose(wb["world_sphere"][0], [1.0, 2.0, 3.0, 1.0], rtol=1e-4)
    assert list(wb["entry_id"]) == [0]


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: rays aimed at silhouettes and edges through the exact map
# ---------------------------------------------------------------------------------------------------------------------------------
MARGINS = [1e-7, 1e-6, 1e-5, 1e-4, 1e-3]
CHAIN_MARGINS = [2.0, 8.0, 32.0]  # multiples of the chain's own rounding scale (ew.Prim.chain_scale), where they fit in the primitive


def _margins(p):
    return MARGINS + [k * p.chain_scale() for k in CHAIN_MARGINS if k * p.chain_scale() < 0.45]


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _aimed_rays(prims, rng, boundary):
    """For every primitive that is not a medium boundary: rays whose exact object-space paths pass each silhouette / edge at signed
    margins of +-MARGINS of its size and of +-CHAIN_MARGINS of its chain's rounding scale, from near (3 sizes), far (1e3 sizes) and, for a sphere, inside it; object-space directions at
    random, along an object axis and along a world axis.  Returns f32 world rays and the primitive each one aims at."""
    O, D, tgt = [], [], []
    for p in prims:
        if boundary[p.id]:
            continue
        Ainv = np.linalg.inv(p.A)
        for kind_dir in range(3):
            for sgn in (1.0, -1.0):
                for m in _margins(p):
                    for dist in (3.0, 1e3, 0.0):
                        if kind_dir == 0:
                            d_obj = _unit(rng.normal(size=3))
                        elif kind_dir == 1:
                            d_obj = np.zeros(3)
                            d_obj[(p.ax if not p.sphere else int(rng.integers(0, 3)))] = -1.0 if rng.random() < 0.5 else 1.0
                        else:  # axis-aligned in the world
                            w = np.zeros(3)
                            w[int(rng.integers(0, 3))] = 1.0
                            d_obj = _unit(p.A @ w)
                        if not p.sphere and abs(d_obj[p.ax]) < 0.05:
                            d_obj[p.ax] = 0.5
                            d_obj = _unit(d_obj)
                        if p.sphere:
                            u = _unit(np.cross(d_obj, _unit(rng.normal(size=3))))
                            P = p.c + p.r * (1.0 - sgn * m) * u
                            if dist == 0.0:  # from inside: the origin on the chord through P, towards its exit
                                Oo = p.c + 0.5 * p.r * (1.0 - sgn * m) * u
                                Oo = Oo - d_obj * np.dot(Oo - P, d_obj)
                                Oo = Oo - d_obj * p.r * 0.1
                            else:
                                Oo = P - d_obj * p.r * dist
                        else:
                            P = np.zeros(3)
                            P[p.ax] = p.k
                            edge_u = rng.random() < 0.5
                            a, b = (p.ua, p.va) if edge_u else (p.va, p.ua)
                            P[a] = p.hi[a] - sgn * m * p.size if rng.random() < 0.5 else p.lo[a] + sgn * m * p.size
                            P[b] = p.lo[b] + (p.hi[b] - p.lo[b]) * rng.uniform(0.1, 0.9)
                            Oo = P - d_obj * p.size * (dist if dist else 0.4)
                        Ow = Ainv @ (Oo - p.b)
                        Dw = Ainv @ d_obj
                        O.append(Ow), D.append(_unit(Dw)), tgt.append(p.id)
    return np.array(O, np.float32), np.array(D, np.float32), np.array(tgt)


def _exact_miss(prims, fs, hit, o, d):
    """True where the list walk's hit is a false positive in exact arithmetic: the ray misses the primitive (or, for a medium, every
    primitive of its boundary) under the chain's exact map."""
    n_prims = fs.n_spheres + fs.n_rects
    ids = [hit] if hit < n_prims else [i for i in range(n_prims) if
                                       (fs.sph_medium[i] if i < fs.n_spheres else fs.rect_medium[i - fs.n_spheres]) == hit - n_prims]
    for i in ids:
        m, _ = prims[i].exact_hit(o[None], d[None], t_min=-np.inf if hit >= n_prims else ew.T_MIN)
        if m[0] >= 0:
            return False
    return True


def _boundary_mask(fs):
    n_prims = fs.n_spheres + fs.n_rects
    return np.array([(fs.sph_medium[i] if i < fs.n_spheres else fs.rect_medium[i - fs.n_spheres]) != ew.NO_XFORM for i in range(n_prims)])


def _tie(prims, fs, h, g, o, d):
    """True where list-walk hit h and search hit g are both primitives the ray meets in exact arithmetic, at exact roots closer than
    f32 can tell apart (their rounding scales at the hit, rt_scene_upload's error model): which of the two comes first is a matter of
    rounding.  Media never count as a tie."""
    n_prims = fs.n_spheres + fs.n_rects
    if h < 0 or g < 0 or h >= n_prims or g >= n_prims:
        return False
    ts, tol = [], 0.0
    for k in (h, g):
        m, t = prims[k].exact_hit(o[None], d[None])
        if not (m[0] >= 0 and np.isfinite(t[0])):
            return False
        ts.append(t[0])
        tol += float(prims[k].rounding_scale(o[None], d[None], t)[0]) * prims[k].size / float(np.linalg.norm(d))
    return abs(ts[0] - ts[1]) <= 2.0 * tol + 1e-6 * max(ts)


GPU_CASES = [("rot_above", 256), ("rot_below", 128), ("rot15", 5), ("cancel1e4", 2), ("cancel1e6", 18), ("cancel1e2", 4),
             ("pivot", 5), ("pivot", 64), ("mix", 18), ("mix", 64), ("mix", 1)]
_seen = {"false positives": 0, "ties": 0}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,depth", GPU_CASES)
def test_searches_agree_on_rays_aimed_at_wrapped_edges(rt, orc, renderer, kind, depth):
    f = rt._ffi
    scene = _finished(rt, kind, depth)
    fs = scene.flat
    prims = ew.primitives(fs)
    boundary = _boundary_mask(fs)
    rng = np.random.default_rng(depth * 31 + KINDS.index(kind))
    o, d, tgt = _aimed_rays(prims, rng, boundary)
    keys = rng.integers(0, 2**32, size=(len(o), 2), dtype=np.uint64).astype(np.uint32)
    # Rays whose fp32 object-space path lies IN the plane of a rectangle (a margin below the rounding of the chain collapses an
    # origin onto the plane, and the direction has no component across it) make XYRect::hit divide 0 by 0: the reference then
    # reports a hit at t = NaN, which the oracle mirrors and the kernels do not.  That is no question of culling; those rays are left out.
    keep = ~np.any([p.in_plane_fp32(o, d) for p in prims], axis=0)
    o, d, tgt, keys = o[keep], d[keep], tgt[keep], keys[keep]
    renderer.upload(scene)
    brute = renderer.debug_bounce(o, d, keys, flags=f.FLAG_BRUTE_FORCE)
    ref = orc.debug_bounce(scene.flat_ptr, o, d, keys, accel=orc.ACCEL_LIST)
    # the list walk is the oracle's, bit for bit — but for the free path inside a medium (hitable.rs:560-570, `neg_inv_density *
    # ln(rand)`), where device and host libm may differ in the last ulp (as in test_gpu_parity._explain_outliers)
    assert np.array_equal(brute["hit"], ref["hit"])
    medium = brute["hit"] >= fs.n_spheres + fs.n_rects
    assert np.array_equal(brute["t"][~medium].view(np.uint32), ref["t"][~medium].view(np.uint32))
    assert np.allclose(brute["t"][medium], ref["t"][medium], rtol=2e-6, atol=0.0), \
        np.abs(brute["t"][medium] / ref["t"][medium] - 1.0).max()
    results = {"tree": renderer.debug_bounce(o, d, keys)}
    results["production"] = renderer.debug_bounce(o, d, path_keys(0, np.arange(len(o)), np.zeros(len(o), np.uint64)),
                                                  flags=f.FLAG_PRODUCTION_KERNELS)
    renderer.set_option("tree_placement", 1)
    renderer.upload(scene)
    results["tree_l2"] = renderer.debug_bounce(o, d, keys)
    renderer.set_option("tree_placement", 0)
    renderer.set_option("general_lds", 1)
    renderer.upload(scene)
    results["tables_hbm"] = renderer.debug_bounce(o, d, keys)
    renderer.set_option("general_lds", 0)
    # the list walk with the production kernels' own RNG keys, for the hit / t comparison (hit and t do not depend on the key except
    # inside a medium, where the scatter distance is drawn)
    prod_ref = renderer.debug_bounce(o, d, path_keys(0, np.arange(len(o)), np.zeros(len(o), np.uint64)), flags=f.FLAG_BRUTE_FORCE)
    n_fp = n_tie = 0
    for name, g in results.items():
        b = prod_ref if name == "production" else brute
        same = (g["hit"] == b["hit"]) & (g["t"].view(np.uint32) == b["t"].view(np.uint32))
        for i in np.flatnonzero(~same):
            h, gh = int(b["hit"][i]), int(g["hit"][i])
            if h >= 0 and _exact_miss(prims, fs, h, o[i], d[i]):
                n_fp += 1
                continue
            assert _tie(prims, fs, h, gh, o[i], d[i]), \
                (kind, depth, name, int(i), "list walk", h, float(b["t"][i]), "search", gh, float(g["t"][i]))
            n_tie += 1
    # rays the exact map puts inside their target by more than fp32 can move them: hit by every search, no later than the exact t
    tp = [prims[int(k)] for k in tgt]
    margin = np.empty(len(o))
    t_ex = np.empty(len(o))
    scale = np.empty(len(o))
    for k in np.unique(tgt):
        sel = tgt == k
        margin[sel], t_ex[sel] = prims[int(k)].exact_hit(o[sel], d[sel])
        scale[sel] = prims[int(k)].rounding_scale(o[sel], d[sel], t_ex[sel])
    sure = (margin > 4.0 * scale) & np.isfinite(t_ex)
    # (a chain that rounds at 1e6 moves a ray by more than a unit-size primitive: no margin is sure there, and the check has nothing to do)
    resolvable = any(32.0 * p.chain_scale() < 0.45 for p in prims if not boundary[p.id])
    assert sure.sum() >= (20 if resolvable else 0), (int(sure.sum()), len(o))
    tol = 1e-5 * t_ex + 4.0 * scale * np.array([p.size for p in tp])
    for name, g in list(results.items()) + [("list walk", brute)]:
        bad = sure & ~((g["hit"] >= 0) & (g["t"].astype(np.float64) <= t_ex + tol))
        assert not bad.any(), (kind, depth, name, [(int(i), int(tgt[i]), float(margin[i]), float(t_ex[i]), int(g["hit"][i]), float(g["t"][i]))
                                                   for i in np.flatnonzero(bad)[:5]])
    _seen["false positives"] += n_fp
    _seen["ties"] += n_tie
    print(f"{kind} depth {depth}: {len(o)} rays ({int((~keep).sum())} in a rectangle's plane left out), {int(sure.sum())} sure hits; "
          f"search / list-walk disagreements: {n_fp} on exact-semantics false positives, {n_tie} on ties within rounding (so far: {_seen})")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,depth", [("cancel1e4", 2), ("rot_above", 128), ("mix", 18)])
def test_candidate_lists_at_wrapped_edges(rt, renderer, kind, depth):
    """Frames from a camera aimed at the edge x = 0.55 of the wrapped XZ rectangle, wherever its chain puts it (eye and target carried
    to the world through the exact map, looking along the edge from above and in front), with and without the per-pixel candidate lists and through
    the list walk, one bounce deep (only primary rays are traced): every pixel that differs holds a primary ray whose list-walk hit is
    an exact-semantics false positive, or two hits a rounding apart."""
    f = rt._ffi
    probe = _finished(rt, kind, depth)
    rect = ew.Prim(probe.flat, probe.flat.n_spheres)  # the XZ rectangle, the first one
    assert not rect.sphere and rect.ax == f.RECT_XZ
    eye, target = ew.object_to_world(rect.ch, np.array([[0.55, 0.6, -2.5], [0.55, -0.9, 0.05]]))
    scene = _finished(rt, kind, depth, eye=tuple(eye), target=tuple(target), vfov=2.0)
    fs = scene.flat
    prims = ew.primitives(fs)
    renderer.upload(scene)
    p = rt.make_params(64, 64, 4, max_depth=1, seed=7)
    imgs = {}
    for name, lists, flags in (("lists", 0, 0), ("tree", 1, 0), ("brute", 0, f.FLAG_BRUTE_FORCE)):
        renderer.set_option("primary_lists", lists)
        p.flags = flags
        imgs[name] = renderer.render(scene.camera, p)[0]
    renderer.set_option("primary_lists", 0)
    n_diff = 0
    for name in ("lists", "tree"):
        diff = (imgs[name].view(np.uint32) != imgs["brute"].view(np.uint32)).any(axis=2)
        jj, ii = np.nonzero(diff)
        n_diff += len(jj)
        for i, j in zip(ii, jj):
            o, d, keys = primary_rays(scene, p, np.full(p.spp, i), np.full(p.spp, j), np.arange(p.spp))
            b = renderer.debug_bounce(o, d, keys, flags=f.FLAG_BRUTE_FORCE)
            g = renderer.debug_bounce(o, d, keys)
            assert any((b["hit"][k] >= 0 and _exact_miss(prims, fs, int(b["hit"][k]), o[k], d[k])) or
                       _tie(prims, fs, int(b["hit"][k]), int(g["hit"][k]), o[k], d[k]) for k in range(p.spp)), (kind, depth, name, i, j)
    # the frame holds the edge: the primary rays hit the rectangle on one side of it and pass it on the other
    jj, ii = np.mgrid[0:p.ny, 0:p.nx]
    o, d, keys = primary_rays(scene, p, np.repeat(ii.ravel(), p.spp), np.repeat(jj.ravel(), p.spp), np.tile(np.arange(p.spp), p.nx * p.ny))
    on_rect = (renderer.debug_bounce(o, d, keys, flags=f.FLAG_BRUTE_FORCE)["hit"] == rect.id).mean()
    assert 0.1 < on_rect < 0.9, on_rect
    print(f"{kind} depth {depth}: {on_rect:.2f} of the primary rays on the rectangle; {n_diff} pixels differ from the list walk, "
          f"each with an exact-semantics false positive or a tie")
