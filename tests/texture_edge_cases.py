"""The scenes, rays and references that tests/test_uv_ref_host.py (CPU, against the oracle) and tests/test_texture_edges.py (GPU) share.
Every scene holds TWO images: a 5 x 3 decoy first and the image under test second, so that the second image's offset into the texel pool
(ImgRec.offset) is in play; the decoy's colours are those of no texel under test (tests/uv_ref.py make_image).  All rays of a case go
through the library in one call; their keys are those the production path derives (seed 0, pixel i, sample 0).  Materials are
MAT_EMISSION unless a case says otherwise: the emitted colour is the texel itself and no random number is drawn."""
import numpy as np

import exact_wrappers
import motion_ref
import quad_ref
import uv_ref
from helpers import path_keys

f32 = np.float32
np_ref = uv_ref.np_ref
DEPTH = 1
IMAGES = {"1x1": (1, 1, False), "1x3": (1, 3, False), "7x5": (7, 5, False), "256x128": (256, 128, True), "1025x513": (1025, 513, False)}
FORMS = {  # name: (centre, radius)
    "unit": ((0.0, 0.0, 0.0), 1.0), "off": ((10.1, -3.3, 7.7), 2.3), "neg": ((1.5, 0.25, -2.0), -0.37),
    "roty": ((1.3, 0.4, -0.8), 0.9), "trans_roty": ((1.3, 0.4, -0.8), 0.9), "moving": ((-0.6, 1.1, 0.7), 0.8)}
BARE, WRAPPED = ("unit", "off", "neg"), ("roty", "trans_roty", "moving")
ROT_DEGREES, OFFSET = 33.0, (4.25, -1.5, 2.75)
CENTER1, SHUTTER = (0.9, 1.6, 0.2), (0.1, 0.9)
DECOY_AT = (170.0, 180.0, 190.0)  # a small sphere that wears the decoy image, off every axis and far from every ray


def keys_for(n):
    return path_keys(0, np.arange(n), np.zeros(n, np.int64))


def _register(rt, name):
    w, h, eight = IMAGES[name]
    rt.register_image("edges/decoy%d.img" % eight, uv_ref.make_image(5, 3, eight, decoy=True))
    rt.register_image("edges/%s.img" % name, uv_ref.make_image(w, h, eight))
    return "edges/decoy%d.img" % eight, "edges/%s.img" % name


def _new_scene(rt, image):
    """-> scene under construction, the texture of the image under test (the decoy image comes first in the pool)"""
    decoy_path, path = _register(rt, image)
    s = rt.Scene.new()
    decoy = s.image_tex(decoy_path)
    tex = s.image_tex(path)
    s.sphere(DECOY_AT, 0.5, s.material(rt._ffi.MAT_EMISSION, tex0=decoy), "decoy")  # flat sphere 0: its image is the first the scene meets
    return s, decoy, tex


def _finish(rt, s, image, sky=None):
    f = rt._ffi
    if sky is None:
        s.set_sky(f.SKY_BLACK, None)
    else:
        s.set_sky(f.SKY_ENV, sky)
    s.set_camera((0.0, 0.0, 0.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), 40.0, 1.0, shutter=SHUTTER)
    scene = s.finish()
    a = scene.arrays()
    w, h, _ = IMAGES[image]
    assert list(a["img_w"]) == [5, w] and list(a["img_h"]) == [3, h], "the decoy is the first image of the pool"
    return scene


# ---- spheres -------------------------------------------------------------------------------------------------------------------------
def sphere_case(rt, form, image, groups, mat="emission"):
    """-> dict(scene, motion (None: static), o, d, keys, group [n] (index into `groups`), on [n, 3]: the local normal of the reference, ref_hit,
    ref_t, w, h, eight_bit, target: the flat index of the sphere)"""
    f = rt._ffi
    w, h, eight = IMAGES[image]
    c, r = FORMS[form]
    s, decoy, tex = _new_scene(rt, image)
    m = s.material(f.MAT_EMISSION if mat == "emission" else f.MAT_DIFFUSE, tex0=tex)
    if form == "moving":
        s.moving_sphere(c, CENTER1, r, m, "target")
    else:
        hnd = s.sphere(c, r, m, "target")
        if form in ("roty", "trans_roty"):
            hnd = s.rotate_y(hnd, ROT_DEGREES)
        if form == "trans_roty":
            s.translate(hnd, OFFSET)
    scene = _finish(rt, s, image)
    a = scene.arrays()
    assert f32(a["sph_r"][1]) == f32(r), "the sphere under test is flat sphere 1"
    chain = exact_wrappers.chain(scene.flat, 1)
    assert len(chain) == {"roty": 1, "trans_roty": 2}.get(form, 0)
    n_each = {g: (6 if g == "axes" else uv_ref.N_GROUP) for g in groups}
    starts = np.cumsum([0] + [n_each[g] for g in groups])
    keys = keys_for(int(starts[-1]))
    O, D, G = [], [], []
    for gi, g in enumerate(groups):
        sl = slice(int(starts[gi]), int(starts[gi + 1]))
        if form == "moving":
            shift = motion_ref.center_at(c, CENTER1, motion_ref.path_time(keys[sl], *SHUTTER)).astype(np.float64) - np.asarray(c, np.float64)
            to_world = lambda p, shift=shift: p + shift
        elif chain:
            to_world = lambda p: exact_wrappers.object_to_world(chain, p)
        else:
            to_world = None
        o, d = uv_ref.group_rays(g, c, r, w, h, seed=len(form) + 10 * w, to_world=to_world)
        O.append(o), D.append(d), G.append(np.full(len(o), gi))
    o, d, grp = np.concatenate(O), np.concatenate(D), np.concatenate(G)
    # the reference's hit: the ray in the sphere's own frame (outermost wrapper first), np_ref's Sphere::hit there
    lo, ld, centre = o, d, np.asarray(c, f32)
    for ty, q in reversed(chain):
        if ty == 0:
            lo = uv_ref.translate_ray(q, lo)
        else:
            lo, ld = uv_ref.rotate_y_ray(q[0], q[1], lo, ld)
    if form == "moving":
        centre = motion_ref.center_at(c, CENTER1, motion_ref.path_time(keys, *SHUTTER))
    hit = uv_ref.sphere_hit(centre, r, lo, ld)
    motion = scene.motion if form == "moving" else None
    return dict(scene=scene, motion=motion, o=o, d=d, keys=keys, group=grp, groups=tuple(groups), on=hit["on"], ref_hit=hit["hit"], ref_t=hit["t"],
                w=w, h=h, eight_bit=eight, target=1, local=(lo, ld, centre, r))


def spot_check_against_np_ref(case, every=97):
    """the vectorised Sphere::hit against tests/golden/np_ref.py's, ray by ray on a sample: t and the outward normal bit for bit"""
    lo, ld, centre, r = case["local"]
    for k in range(0, len(lo), every):
        c = centre[k] if centre.ndim == 2 else centre
        h = np_ref.sphere_hit(np_ref.v3(*c), f32(r), np_ref.v3(*lo[k]), np_ref.v3(*ld[k]), f32(1e-3), uv_ref.FLT_MAX)
        assert (h is not None) == bool(case["ref_hit"][k]), k
        if h is not None:
            assert f32(h["t"]).view(np.uint32) == case["ref_t"][k].view(np.uint32), k
            assert np.array_equal(np.array(h["on"], f32).view(np.uint32), case["on"][k].view(np.uint32)), k


def group_statistics(case):
    """The coverage conditions of every group of a sphere case, on the reference alone.  -> {group: dict(hits, ambiguous, nan_row, ...)}, cand"""
    w, h = case["w"], case["h"]
    cand = uv_ref.candidates(case["on"], w, h)
    out = {}
    for gi, g in enumerate(case["groups"]):
        sel = case["group"] == gi
        sub = {k: v[sel] for k, v in cand.items()}
        st, i0, j0 = uv_ref.check_group(g, sub, case["ref_hit"][sel], w, h)
        ny = case["on"][sel][case["ref_hit"][sel], 1]
        single = sub["single"][case["ref_hit"][sel]]
        if g == "random" and (w, h) == (7, 5):
            st["texels"] = len(set(zip(i0[single].tolist(), j0[single].tolist())))
            assert st["texels"] >= 0.95 * w * h, (g, st)
        if g == "pole_south":
            st["below_-1"], st["bottom_row"] = float((ny < -1).mean()), float((j0 == h - 1).mean())
            assert st["below_-1"] >= 0.05 and (h == 1 or st["bottom_row"] >= 0.05), (g, st)
            assert h == 1 or (j0[ny < -1] == 0).all()  # the NaN row is the top one
        if g == "pole_north":
            st["above_1"] = float((ny > 1).mean())
            assert st["above_1"] >= 0.05, (g, st)
        if g == "seam" and w > 1:
            assert (i0[single] == 0).any() and (i0[single] == w - 1).any(), (g, st)
        if g == "border" and w > 1 and h > 1:
            # decided rays fall on both sides of a border: among them, neighbouring columns and neighbouring rows both occur
            ii, jj = i0[single], j0[single]
            assert (np.diff(np.unique(ii)) == 1).sum() >= min(w, 4) - 1 and (np.diff(np.unique(jj)) == 1).sum() >= min(h, 4) - 1, (g, st)
        out[g] = st
    return out, cand


# ---- sky -----------------------------------------------------------------------------------------------------------------------------
def sky_case(rt, image):
    w, h, eight = IMAGES[image]
    s, decoy, tex = _new_scene(rt, image)
    scene = _finish(rt, s, image, sky="edges/%s.img" % image)
    assert scene.arrays()["sky_image"] == 1
    dirs = uv_ref.sky_directions(seed=w)
    names = list(dirs)
    d = np.concatenate([dirs[k] for k in names])
    grp = np.concatenate([np.full(len(dirs[k]), i) for i, k in enumerate(names)])
    o = np.zeros_like(d)
    l2 = np_ref.dot(uv_ref._cols(d), uv_ref._cols(d))
    assert ((l2 >= f32(0.9999981)) & (l2 <= f32(1.000002))).all(), "every direction passes the near-one window of main.rs:39"
    return dict(scene=scene, motion=None, o=o, d=d, keys=keys_for(len(o)), group=grp, groups=tuple(names), w=w, h=h, eight_bit=eight)


def sky_statistics(case):
    w, h = case["w"], case["h"]
    cand = uv_ref.candidates(case["d"], w, h, sky=True)
    out = {}
    for gi, g in enumerate(case["groups"]):
        sel = case["group"] == gi
        out[g] = {"rays": int(sel.sum()), "ambiguous": float((~cand["single"][sel]).mean()), "nan_row": float(cand["nan_row"][sel].mean())}
        if g != "forced":
            assert out[g]["ambiguous"] <= 0.005, (g, out[g])
    k = np.nonzero(case["group"] == case["groups"].index("forced"))[0]
    assert cand["single"][k[:4]].all() and (cand["I"][k].min(axis=1) == cand["I"][k].max(axis=1))[:6].all()  # (d.y = 0 is a row border of an even height)
    # (0, +-nextafter(1, 2), 0): acos is NaN, row 0 — straight DOWN reads the zenith row; (0, +-nextafter(1, 0), 0): top and bottom row
    assert list(cand["nan_row"][k]) == [True, True, False, False, False, False, False, False]
    assert list(cand["j0"][k[:4]]) == [0, 0, 0, h - 1]
    # the seam: (-1, 0, +0) reads column w - 1 (u = 1 through the sky's 1 - uv.x and the min), (-1, 0, -0) column 0
    assert list(cand["i0"][k[4:6]]) == [w - 1, 0]
    for g, row in (("cone_up", 0), ("cone_down", h - 1)):  # (normalised, the cones' y is exactly +-1: only the forced directions are longer)
        sel = case["group"] == case["groups"].index(g)
        assert (cand["j0"][sel] == row).all() and len(np.unique(cand["i0"][sel])) >= min(w, 5)
    return out, cand


def frame_case(rt, image, down):
    """an 8 x 8 frame, 1 spp, max_depth 1, the camera at the origin looking straight down (up): every pixel is the sky"""
    s, decoy, tex = _new_scene(rt, image)
    f = rt._ffi
    s.set_sky(f.SKY_ENV, "edges/%s.img" % image)
    s.set_camera((0.0, 0.0, 0.0), (0.0, -1.0 if down else 1.0, 0.0), (1.0, 0.0, 0.0), 0.02, 1.0)  # a field of view of 0.02 degrees: every direction's y rounds to +-1 or a neighbour of it
    return s.finish()


# ---- rectangles, a box, a planar set ---------------------------------------------------------------------------------------------------------
RECTS = [(2, (1.0, -1.0, -2.0), (3.0, 0.5, -2.0)), (1, (-2.0, 1.5, -1.0), (0.0, 1.5, 3.0)), (0, (-3.5, -2.0, 0.5), (-3.5, 2.0, 1.0))]  # XY, XZ, YZ
BOX = ((4.0, 1.125, -3.0), (5.5, 2.25, -2.0))  # (no face in the plane of an axis-parallel ray: 0 / 0 is a hit with t = NaN in the reference)
QUAD = ((-1.0, -1.0, 5.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0))      # alpha = (p.x + 1) / 2, beta = (p.y + 1) / 2, exactly
TRIANGLE = ((3.0, -1.0, 5.0), (5.0, -1.0, 5.0), (3.0, 1.0, 5.0))  # corners a, b, c: u = (2, 0, 0), v = (0, 2, 0)
N_INTERIOR = 5000


def _axis_rays(axis, mn, mx, rng, n_interior=N_INTERIOR):
    """rays along -axis from 4 units in front of the plane: on the four borders and the four corners (u, v in {0, 1} exactly: the origin's two
    other coordinates are the rectangle's own), and n_interior at random inside"""
    ua, va = ((1, 2), (0, 2), (0, 1))[axis]
    pts = []
    for fu in (0.0, 1.0):
        for fv in (0.0, 1.0):
            pts.append((mn[ua] + fu * (mx[ua] - mn[ua]), mn[va] + fv * (mx[va] - mn[va])))
    for k in range(64):
        tu, tv = rng.uniform(mn[ua], mx[ua]), rng.uniform(mn[va], mx[va])
        pts += [(mn[ua], tv), (mx[ua], tv), (tu, mn[va]), (tu, mx[va])]
    pts += list(zip(rng.uniform(mn[ua], mx[ua], n_interior), rng.uniform(mn[va], mx[va], n_interior)))
    pts = np.array(pts)
    o = np.zeros((len(pts), 3))
    o[:, ua], o[:, va], o[:, axis] = pts[:, 0], pts[:, 1], mn[axis] + 4.0
    d = np.zeros((len(pts), 3))
    d[:, axis] = -1.0
    return o.astype(f32), d.astype(f32)


def rect_uv(axis, mn, mx, o, d):
    """np_ref.rect_hit for rays [n, 3]: (hit, t, u, v)"""
    mn, mx = np.asarray(mn, f32), np.asarray(mx, f32)
    ua, va = ((1, 2), (0, 2), (0, 1))[axis]
    with np.errstate(all="ignore"):
        t = ((mn[axis] - o[:, axis]) / d[:, axis]).astype(f32)
        p = (o + (d * t[:, None]).astype(f32)).astype(f32)
        hit = ~((t < f32(1e-3)) | (t > uv_ref.FLT_MAX)) & ~((p[:, ua] < mn[ua]) | (p[:, ua] > mx[ua]) | (p[:, va] < mn[va]) | (p[:, va] > mx[va]))
        u = ((p[:, ua] - mn[ua]) / (mx[ua] - mn[ua])).astype(f32)
        v = ((p[:, va] - mn[va]) / (mx[va] - mn[va])).astype(f32)
    return hit, t, u, v, p


def flat_case(rt, image="7x5"):
    """One rectangle per axis, a box and a planar set of one quad and one triangle, all wearing the image.  -> dict(scene, quads, o, d, keys,
    want_hit, want_t, want_colour [n, 3]: np_ref.rect_hit + np_ref.image_value and quad_ref, vectorised, i, j: the texel read)"""
    f = rt._ffi
    w, h, eight = IMAGES[image]
    s, decoy, tex = _new_scene(rt, image)
    m = s.material(f.MAT_EMISSION, tex0=tex)
    for axis, mn, mx in RECTS:
        s.rect(axis, mn, mx, m)
    s.gbox(BOX[0], BOX[1], m)
    s.quad(*QUAD, m)
    s.triangle(*TRIANGLE, m)
    scene = _finish(rt, s, image)
    a = scene.arrays()
    nr = scene.flat.n_rects
    assert nr == 9 and scene.flat.n_spheres == 1 and scene.quads.n == 2
    rng = np.random.default_rng(5)
    O, D = [], []
    for axis, mn, mx in RECTS:
        o, d = _axis_rays(axis, mn, mx, rng)
        O.append(o), D.append(d)
    # the box: from a shell around it at random points inside it
    cb, hb = (np.array(BOX[0]) + np.array(BOX[1])) / 2, (np.array(BOX[1]) - np.array(BOX[0])) / 2
    v = rng.normal(size=(N_INTERIOR, 3))
    o = (cb + 6.0 * v / np.linalg.norm(v, axis=1)[:, None]).astype(f32)
    O.append(o), D.append(uv_ref.normalize_f32((cb + rng.uniform(-0.9, 0.9, (N_INTERIOR, 3)) * hb - o).astype(f32)))
    # the quad and the triangle: along -z onto the edges (alpha, beta in {0, 1}), the corners, and inside
    qmn, qmx = (-1.0, -1.0, 5.0), (1.0, 1.0, 5.0)
    o, d = _axis_rays(2, qmn, qmx, rng, 1500)
    O.append(o), D.append(d)
    o, d = _axis_rays(2, (3.0, -1.0, 5.0), (5.0, 1.0, 5.0), rng, 3000)  # (half of the interior ones miss the triangle: alpha + beta > 1)
    O.append(o), D.append(d)
    o, d = np.concatenate(O), np.concatenate(D)
    n = len(o)
    # reference: rectangles in entry order (the closest wins; none of these rays meets two at the same t), then the planar set
    best_t, best = np.full(n, uv_ref.FLT_MAX, f32), np.full(n, -1, np.int64)
    U, V = np.zeros(n, f32), np.zeros(n, f32)
    for r in range(nr):
        hit, t, u, v, _ = rect_uv(int(a["rect_axis"][r]), a["rect_min"][3 * r:3 * r + 3], a["rect_max"][3 * r:3 * r + 3], o, d)
        take = hit & (t < best_t)
        assert not (hit & (t == best_t)).any() and not np.isnan(t[hit]).any()
        best_t[take], best[take], U[take], V[take] = t[take], 1 + r, u[take], v[take]
    base = 1 + nr + scene.flat.n_media
    q, qu, qv = (np.array(x, f32).reshape(1, 3) for x in QUAD)
    ta, tb, tc = (np.array(x, f32) for x in TRIANGLE)
    Q, QU, QV = np.concatenate([q, ta[None]]), np.concatenate([qu, (tb - ta)[None]]), np.concatenate([qv, (tc - ta)[None]])
    ph, pt, al, be = quad_ref.closest(Q, QU, QV, [quad_ref.QUAD, quad_ref.TRIANGLE], o, d, base=base, t0=best_t, hit0=best)
    planar = ph >= base
    best[planar], best_t[planar], U[planar], V[planar] = ph[planar], pt[planar], al[planar], be[planar]
    i, j = uv_ref.texel_index(U, V, w, h)
    img = uv_ref.make_image(w, h, eight)
    colour = np.where((best >= 0)[:, None], img[j, i], f32(0.0)).astype(f32)
    return dict(scene=scene, quads=scene.quads, o=o, d=d, keys=keys_for(n), want_hit=best, want_t=best_t, want_colour=colour, i=i, j=j, u=U, v=V,
                w=w, h=h, n_rects=nr, base=base, image=img)


def flat_statistics(X):
    hit = X["want_hit"]
    nr, base, w, h = X["n_rects"], X["base"], X["w"], X["h"]
    st = {"rect_hits": [int((hit == 1 + r).sum()) for r in range(nr)], "quad_hits": int((hit == base).sum()), "triangle_hits": int((hit == base + 1).sum()),
          "misses": int((hit < 0).sum())}
    assert min(st["rect_hits"][:3]) >= N_INTERIOR and min(st["rect_hits"][3:]) >= 100 and st["quad_hits"] >= 1500 and st["triangle_hits"] >= 1000, st
    groups = [(hit == 1 + r, True) for r in range(3)] + [((hit > 3) & (hit < base), False), (hit == base, True)]  # three rectangles, the box, the quad
    for sel, edges in groups:
        assert len(set(zip(X["i"][sel].tolist(), X["j"][sel].tolist()))) == w * h, "every texel of the image is read"
        u, v = X["u"][sel], X["v"][sel]
        if edges:  # the borders and corners: u, v of exactly 0 and 1
            assert all(((u == a) & (v == b)).any() for a in (0, 1) for b in (0, 1)), "the four corners"
            assert ((u == 1) & (X["i"][sel] == w - 1)).any() and ((v == 0) & (X["j"][sel] == h - 1)).any() and ((v == 1) & (X["j"][sel] == 0)).any()
    t = hit == base + 1
    assert ((X["u"][t] == 0).any() and (X["v"][t] == 0).any() and ((X["u"][t] == 1) & (X["v"][t] == 0)).any()), "the triangle's edges and a corner"
    return st


def spot_check_flat_against_np_ref(X, every=53):
    """rectangle hits against np_ref.rect_hit + np_ref.image_value, planar hits against np_ref.image_value on quad_ref's (alpha, beta)"""
    a = X["scene"].arrays()
    for k in range(0, len(X["o"]), every):
        hit = int(X["want_hit"][k])
        if hit < 1:
            continue
        o, d = np_ref.v3(*X["o"][k]), np_ref.v3(*X["d"][k])
        if hit < X["base"]:
            r = hit - 1
            rec = np_ref.rect_hit(int(a["rect_axis"][r]), np_ref.v3(*a["rect_min"][3 * r:3 * r + 3]), np_ref.v3(*a["rect_max"][3 * r:3 * r + 3]), o, d,
                                  f32(1e-3), uv_ref.FLT_MAX)
            assert rec is not None and f32(rec["t"]).view(np.uint32) == X["want_t"][k].view(np.uint32), k
            uv = rec["uv"]
        else:
            uv = (X["u"][k], X["v"][k])
        assert np.array_equal(np.array(np_ref.image_value(X["image"], uv), f32).view(np.uint32), X["want_colour"][k].view(np.uint32)), k


# ---- checker --------------------------------------------------------------------------------------------------------------------------
ODD, EVEN = (0.125, 0.25, 0.5), (0.75, 0.875, 1.0)  # `sines < 0` takes ODD (texture.rs:44-48)
FLOOR = (1, (-8.0, 0.0, -8.0), (8.0, 0.0, 8.0))
FAR = {"1e5": ((6.0e4, 5.0e4, 6.2e4), 1000.0), "1e6": ((-6.1e5, 5.2e5, 5.9e5), 1000.0)}


def checker_case(rt, where):
    """where: "floor" (an XZ rectangle at y = 0 through the origin) or a key of FAR (a sphere of r = 1000 at |c| = 1e5 / 1e6: arguments 10 p of
    1e5 .. 1e7 need sin's whole range reduction).  -> dict(scene, o, d, keys, ref_hit, ref_t, negative, decided, straight: the rays whose
    hit has a coordinate of exactly +-0)"""
    f = rt._ffi
    s, decoy, tex = _new_scene(rt, "7x5")
    m = s.material(f.MAT_EMISSION, tex0=s.checker_tex(ODD, EVEN))
    rng = np.random.default_rng(11)
    s.sphere((-DECOY_AT[0], DECOY_AT[1], DECOY_AT[2]), 0.5, s.material(f.MAT_EMISSION, tex0=tex), "image")  # flat sphere 1
    if where == "floor":
        s.rect(*FLOOR, m)
        n = 4000
        # straight down and straight up: p.y = o.y + d.y t is exactly +0; x (z) of -0 with a direction component of -0 stays -0
        x, z = rng.uniform(-7.5, 7.5, n), rng.uniform(-7.5, 7.5, n)
        x[:200], z[200:400] = -0.0, -0.0
        x[400:500], z[400:500] = 0.0, 0.0
        o1 = np.stack([x, np.where(np.arange(n) % 2 == 0, 2.0, -2.0), z], axis=1).astype(f32)
        d1 = np.zeros((n, 3), f32)
        d1[:, 1] = -np.sign(o1[:, 1])
        d1[:200, 0], d1[200:400, 2] = -0.0, -0.0
        # oblique rays: p.y is whatever o.y + d.y t rounds to
        o2 = np.stack([rng.uniform(-7, 7, n), rng.choice([-3.0, 2.5], n), rng.uniform(-7, 7, n)], axis=1).astype(f32)
        tgt = np.stack([rng.uniform(-7.5, 7.5, n), np.zeros(n), rng.uniform(-7.5, 7.5, n)], axis=1)
        d2 = uv_ref.normalize_f32((tgt - o2).astype(f32))
        o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
        scene = _finish(rt, s, "7x5")
        hit, t, _, _, p = rect_uv(FLOOR[0], FLOOR[1], FLOOR[2], o, d)
        straight = np.arange(len(o)) < n
        assert (p[straight, 1] == 0).all() and hit[straight].all()
        assert np.signbit(p[:200, 0]).all() and np.signbit(p[200:400, 2]).all()
        straight = (p == 0).any(axis=1) & hit  # (o.y + d.y t cancels exactly for most of the oblique rays too: a floor at y = 0 is one colour)
        assert 0.02 < (~straight[n:]).mean() < 0.5
        target = 2  # (the rectangle follows the two spheres in the flat index order)
    else:
        c, r = FAR[where]
        s.sphere(c, r, m, "far")
        scene = _finish(rt, s, "7x5")
        o, d = uv_ref.group_rays("random", c, r, 7, 5, seed=3)
        H = uv_ref.sphere_hit(np.asarray(c, f32), r, o, d)
        hit, t, p = H["hit"], H["t"], H["p"]
        straight = np.zeros(len(o), bool)
        target = 2
    negative, decided = uv_ref.checker(p)
    return dict(scene=scene, o=o, d=d, keys=keys_for(len(o)), ref_hit=hit, ref_t=t, negative=negative, decided=decided, straight=straight, p=p, target=target)


def checker_statistics(X, where):
    k = X["ref_hit"]
    st = {"hits": int(k.sum()), "undecided": float((~X["decided"][k]).mean()), "negative": float(X["negative"][k].mean())}
    assert st["hits"] >= 0.9 * len(k) and st["undecided"] <= 0.005, st
    assert not X["negative"][X["straight"]].any() and X["decided"][X["straight"]].all()  # a factor of +-0: not negative
    if where == "floor":
        assert 0.2 < X["negative"][k & ~X["straight"]].mean() < 0.8, st  # off the plane by an ulp, rays see both colours: the zeros are what holds the others
    else:
        assert 0.4 < st["negative"] < 0.6, st
        assert np.abs(X["p"][k] * f32(10.0)).min() >= 1e5
    return st


def checker_colour(X):
    return np.where(X["negative"][:, None], np.array(ODD, f32), np.array(EVEN, f32)).astype(f32)
