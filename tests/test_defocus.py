"""Thin-lens camera on the GPU (rt_set_lens).  Pinhole frames do not move by one bit; lens rays are the numpy restatement's
(tests/lens_ref.py) bit for bit; every closest-hit search agrees with a lens on; the candidate lists' lens bound is conservative;
the blur has the width a thin lens gives it; invalid lenses are refused."""
import os
import sys

import numpy as np
import pytest

import lens_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import np_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def lensed(renderer):
    """the session's Renderer, handed back as a pinhole camera whatever the test left behind"""
    yield renderer
    renderer.set_lens(None)


def _bits(img):
    return img.view(np.uint32)


def _same(a, b, what=""):
    assert np.array_equal(_bits(a[0]), _bits(b[0])), what
    if a[1] is not None or b[1] is not None:
        assert np.array_equal(a[1], b[1]), what
    assert a[2].n_rays == b[2].n_rays and list(a[2].rays_per_depth) == list(b[2].rays_per_depth), what


# ---- 1. the pinhole frames do not move ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nx,ny,spp,depth,lens", [("sphere_scene", 160, 90, 8, 12, (0.05, 10.0)),  # lists + grid
                                                       ("cornell_box", 96, 96, 8, 12, (10.0, 800.0)),   # general
                                                       ("final_scene", 96, 96, 6, 8, (10.0, 630.0))])   # general, tree in L2
def test_pinhole_frames_do_not_move(rt, name, nx, ny, spp, depth, lens):
    """A context that never saw a lens, one given {0, 7}, and one given a real lens and then None render the same bits."""
    scene = rt.Scene.build(name, nx / ny)
    r = rt.Renderer(0)
    try:
        r.upload(scene)
        for spp_slice in (0, 3):
            p = rt.make_params(nx, ny, spp, max_depth=depth, seed=7, spp_slice=spp_slice)
            never = r.render(scene.camera, p, want_rgb8=True)
            r.set_lens(rt.RtLens(0.0, 7.0))
            zero = r.render(scene.camera, p, want_rgb8=True)
            r.set_lens(lens)
            with_lens = r.render(scene.camera, p, want_rgb8=True)
            r.set_lens(None)
            back = r.render(scene.camera, p, want_rgb8=True)
            _same(never, zero, (name, spp_slice))
            _same(never, back, (name, spp_slice))
            assert not np.array_equal(_bits(with_lens[0]), _bits(never[0]))
    finally:
        r.close()


# ---- 2. the lens rays, exactly -----------------------------------------------------------------------------------------------
SPHERES = [((0.0, 0.0, -4.0), 1.0), ((-1.6, 0.4, -6.5), 0.9), ((1.1, -0.5, -2.5), 0.45)]
CAM = ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 40.0, 1.5)


def _black_spheres(rt, spheres, cam):
    f = rt._ffi
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    m = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.0, 0.0, 0.0)))
    for c, r in spheres:
        s.sphere(c, r, m, "s")
    s.set_camera(*cam)
    return s.finish()


def _misses(o, d, spheres):
    """no Sphere::hit (np_ref.sphere_hit, hitable.rs:75-102) in [1e-3, FLT_MAX] for any sphere"""
    f = np.float32
    out = np.ones(len(o), bool)
    for k in range(len(o)):
        ok, dk = tuple(f(x) for x in o[k]), tuple(f(x) for x in d[k])
        for c, r in spheres:
            if np_ref.sphere_hit(np_ref.v3(*c), f(r), ok, dk, f(1e-3), f(3.4028235e38)) is not None:
                out[k] = False
                break
    return out


def _expected(scene, p, lens, spheres):
    """max_depth 0, black diffuse spheres under the gradient sky: the in-order float32 sum of sky(d) over the missing samples / spp"""
    jj, ii = np.meshgrid(np.arange(p.ny), np.arange(p.nx), indexing="ij")
    i, j = ii.ravel(), jj.ravel()
    acc = np.zeros((len(i), 3), np.float32)
    for s in range(p.spp):
        o, d, _ = lens_ref.lens_rays(scene.camera, p, i, j, np.full(len(i), s), lens[0], lens[1])
        acc = (acc + np.where(_misses(o, d, spheres)[:, None], lens_ref.sky_gradient(d), np.float32(0.0))).astype(np.float32)
    return (acc / np.float32(p.spp)).astype(np.float32).reshape(p.ny, p.nx, 3)


@pytest.mark.parametrize("lens", [(0.0, 1.0), (0.05, 1.5), (0.05, 3.0), (0.05, 9.0), (0.5, 1.5), (0.5, 3.0), (0.5, 9.0)])
def test_lens_rays_are_the_restatement_bit_for_bit(rt, lensed, lens):
    """Focus in front of all spheres (1.5), at the front of the middle one (3.0) and behind all (9.0).  1 spp (no candidate lists) and
    8 spp (lists on): every pixel bit for bit.  (The 8-spp frames once had an allowance of 2 ulp; a radiance slot is written once and
    k_resolve adds the samples in order, so nothing can differ, and on the MI355X nothing does: the largest difference measured is 0.)"""
    scene = _black_spheres(rt, SPHERES, CAM)
    lensed.upload(scene)
    lensed.set_lens(lens)
    for nx, ny, spp in ((64, 40, 1), (40, 24, 8)):
        p = rt.make_params(nx, ny, spp, max_depth=0, seed=21)
        img, _, st = lensed.render(scene.camera, p)
        want = _expected(scene, p, lens, SPHERES)
        assert st.n_rays == nx * ny * spp
        hit = (want == 0).all(axis=2)
        assert 0.03 < hit.mean() < 0.9  # spheres and sky both in the frame
        ulp = np.abs(img.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
        print("lens %r, %d spp: the largest difference is %d ulp" % (lens, spp, ulp))
        assert ulp == 0, (lens, spp, ulp)
        if spp == 8:
            assert lensed.render_parts()["primary_lists_overflow"] >= 0  # the frame had candidate lists


# ---- 3. every search path agrees with a lens on --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nx,ny,lens", [("sphere_scene", 96, 54, (0.05, 10.0)),  # the book's cover lens
                                             ("pbr_sweep_scene", 96, 54, (0.4, 28.8)), ("cornell_box", 64, 64, (12.0, 800.0))])
def test_every_search_path_agrees_with_a_lens(rt, lensed, name, nx, ny, lens):
    from ray_tracing_in_one_weekend_amd import shard
    scene = rt.Scene.build(name, nx / ny)
    lensed.upload(scene)
    p = rt.make_params(nx, ny, 6, max_depth=8, seed=11)
    pinhole = lensed.render(scene.camera, p)
    lensed.set_lens(lens)
    ref = lensed.render(scene.camera, p)
    assert not np.array_equal(_bits(ref[0]), _bits(pinhole[0]))
    brute = rt.make_params(nx, ny, 6, max_depth=8, seed=11, flags=rt._ffi.FLAG_BRUTE_FORCE)  # list walk, primaries materialised
    _same(ref, lensed.render(scene.camera, brute), (name, "list walk"))
    for opt, val in (("grid", 1), ("primary_lists", 1), ("materialise_primaries", 1), ("pixel_order", 1), ("pixel_order", 2)):
        lensed.set_option(opt, val)
        got = lensed.render(scene.camera, p)
        lensed.set_option(opt, 0)
        _same(ref, got, (name, opt, val))
    parts = [lensed.render(scene.camera, rt.make_params(nx, ny, 6, max_depth=8, seed=11, shard_band=8, shard_count=2, shard_id=k,
                                                        spp_slice=4))[0] for k in range(2)]
    assert np.array_equal(_bits(shard.deinterleave(parts, ny, 8, 2)), _bits(ref[0]))
    m = rt.MultiRenderer([0, 0], copy_gather=True)
    try:
        m.upload(scene)
        m.set_lens(lens)
        img, _, st = m.render(scene.camera, p)
        assert np.array_equal(_bits(img), _bits(ref[0])) and st.n_rays == ref[2].n_rays
    finally:
        m.close()


# ---- 4. the candidate lists' lens bound is conservative ------------------------------------------------------------------------
FOCUS = 5.0
CLOUDS = [  # (seed, spheres, where, lens_radius / focus)
    (1, 200, "focal", 0.005), (2, 400, "focal", 0.005), (3, 200, "focal", 0.05), (4, 300, "far", 0.005), (5, 200, "far", 0.05),
    (6, 200, "near", 0.05), (7, 600, "near", 0.005), (8, 1500, "focal", 0.02)]


def _cloud(rt, seed, n, where, R):
    """n small spheres at the plane of focus (with four of them inside 2R of the eye: "near") or 3-6 focus distances behind it, in the
    view of a camera at the origin looking down -z (vfov 30, aspect 1.5)"""
    f = rt._ffi
    g = np.random.default_rng(seed)
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    mats = [s.material(f.MAT_DIFFUSE, tex0=s.constant_tex(tuple(float(x) for x in g.uniform(0.2, 0.9, 3)))) for _ in range(4)]
    z = g.uniform(0.9, 1.1, n) * FOCUS if where != "far" else g.uniform(3.0, 6.0, n) * FOCUS
    c = np.stack([g.uniform(-1, 1, n) * 0.42 * z, g.uniform(-1, 1, n) * 0.28 * z, -z], axis=1)
    rad = g.uniform(0.004, 0.01, n) * z
    if where == "near":  # a few of them within 2R of the eye, in front of it, the rest at the plane of focus
        k = 4
        v = g.normal(size=(k, 3))
        v[:, 2] = -np.abs(v[:, 2])
        c[:k] = v / np.linalg.norm(v, axis=1, keepdims=True) * g.uniform(1.2, 2.0, (k, 1)) * R
        rad[:k] = g.uniform(0.1, 0.25, k) * R
    for ci, ri in zip(c, rad):
        s.sphere(tuple(float(x) for x in ci), float(ri), mats[int(g.integers(0, 4))], "s")
    s.set_camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 30.0, 1.5)
    return s.finish()


@pytest.mark.parametrize("seed,n,where,ratio", CLOUDS)
def test_candidate_lists_hold_every_sphere_a_lens_ray_can_hit(rt, lensed, seed, n, where, ratio):
    R = ratio * FOCUS
    scene = _cloud(rt, seed, n, where, R)
    lensed.upload(scene)
    lensed.set_lens((R, FOCUS))
    p = rt.make_params(96, 64, 4, max_depth=2, seed=seed)
    on = lensed.render(scene.camera, p)
    overflow = lensed.render_parts()["primary_lists_overflow"]
    lensed.set_option("primary_lists", 1)
    off = lensed.render(scene.camera, p)
    lensed.set_option("primary_lists", 0)
    _same(on, off, (seed, where, ratio))
    assert 0 <= overflow <= 96 * 64
    assert (on[0].max(axis=2) < 0.95 * on[0].max()).mean() > 0.02  # spheres in the frame
    if where != "near" and ratio <= 0.005:
        assert overflow <= 0.75 * 96 * 64, overflow  # most pixels keep a list: the comparison above tested them


# ---- 5. it blurs as a thin lens should ---------------------------------------------------------------------------------------
def _silhouette_depth(c, r, side):
    """depth along -z of the silhouette point of sphere (c, r) seen from the origin, in the plane y = 0, on side -1 (left) / +1"""
    c = np.array(c, float)
    dist = np.linalg.norm(c)
    u = c / dist
    p0 = u * (dist * dist - r * r) / dist
    rho = r * np.sqrt(dist * dist - r * r) / dist
    perp = np.array([-u[2], 0.0, u[0]])
    if perp[0] * side < 0:
        perp = -perp
    return -(p0 + rho * perp)[2]


def _width_10_90(q):
    """10 %-90 % width, in pixels, of a profile falling from 1 to 0 (first crossings, linear between pixel centres)"""
    def cross(level):
        k = int(np.argmax(q < level))
        assert k > 0
        return (k - 1) + (q[k - 1] - level) / (q[k - 1] - q[k])
    return cross(0.1) - cross(0.9)


def _disc_edge_width(D):
    """10 %-90 % width of a straight edge blurred by a uniform disc of diameter D pixels and averaged over the 1-pixel footprint"""
    x = np.linspace(-D / 2 - 3.0, D / 2 + 3.0, 60001)
    if D > 0:
        s = np.clip(x / (D / 2), -1.0, 1.0)
        F = 0.5 + (s * np.sqrt(1 - s * s) + np.arcsin(s)) / np.pi
    else:
        F = (x >= 0).astype(float)
    k = int(round(0.5 / (x[1] - x[0])))
    G = np.convolve(F, np.ones(2 * k + 1) / (2 * k + 1), mode="same")[k:-k]
    xs = x[k:-k]
    return np.interp(0.9, G, xs) - np.interp(0.1, G, xs)


def test_defocus_blur_has_the_width_of_a_thin_lens(rt, lensed):
    """Two black spheres under the sky, max_depth 0, 256 spp: the edge of the one at half the focus distance spreads like a uniform disc
    of diameter 2R |1/z - 1/f| ny / (2 tan(vfov / 2)) pixels (within 15 %); the edge of the one at the focus distance stays sharp."""
    nx, ny, spp, vfov = 300, 200, 256, 20.0
    focus, R = 10.0, 0.1
    near, far = ((-0.5, 0.0, -5.0), 0.45), ((1.3, 0.0, -10.0), 0.8)
    cam = ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), vfov, nx / ny)
    scene = _black_spheres(rt, [near, far], cam)
    sky = _black_spheres(rt, [((-0.5, 0.0, 5.0), 0.45), ((1.3, 0.0, 10.0), 0.8)], cam)  # the same spheres behind the eye: sky only
    p = rt.make_params(nx, ny, spp, max_depth=0, seed=3)
    lensed.upload(sky)
    S = lensed.render(sky.camera, p)[0]
    lensed.upload(scene)
    pin = lensed.render(scene.camera, p)[0]
    lensed.set_lens((R, focus))
    img = lensed.render(scene.camera, p)[0]
    rows = slice(97, 103)  # around the spheres' centre row
    q_lens, q_pin = (img[rows, :, 0] / S[rows, :, 0]).mean(axis=0), (pin[rows, :, 0] / S[rows, :, 0]).mean(axis=0)
    px = ny / (2.0 * np.tan(np.radians(vfov) / 2.0))
    near_col = int(nx / 2 + near[0][0] / -near[0][2] * px)  # the near sphere's centre column: its left edge lies before it
    far_col = int(nx / 2 + far[0][0] / -far[0][2] * px)
    D_near = 2 * R * abs(1 / _silhouette_depth(*near, -1) - 1 / focus) * px
    D_far = 2 * R * abs(1 / _silhouette_depth(*far, +1) - 1 / focus) * px
    assert D_near > 8.0 and D_far < 0.5
    w_near = _width_10_90(q_lens[:near_col])
    assert abs(w_near / _disc_edge_width(D_near) - 1.0) < 0.15, (w_near, _disc_edge_width(D_near), D_near)
    assert _width_10_90(q_pin[:near_col]) < 2.0  # (the pinhole edge of the same sphere is sharp: a 1-pixel box and its curvature)
    w_far_lens, w_far_pin = _width_10_90(q_lens[::-1][:nx - far_col]), _width_10_90(q_pin[::-1][:nx - far_col])
    assert w_far_lens <= w_far_pin + 1.0, (w_far_lens, w_far_pin)


# ---- 6. validation -------------------------------------------------------------------------------------------------------------
def test_invalid_lenses_are_refused_and_the_previous_one_stays(rt, lensed):
    scene = _black_spheres(rt, SPHERES, CAM)
    lensed.upload(scene)
    p = rt.make_params(48, 32, 2, max_depth=0, seed=5)
    lensed.set_lens((0.3, 4.0))
    before = lensed.render(scene.camera, p)[0]
    nan, inf = float("nan"), float("inf")
    for bad in ((nan, 4.0), (0.3, nan), (-0.1, 4.0), (0.3, 0.0), (0.3, -2.0), (inf, 4.0), (0.3, inf), (0.0, nan)):
        with pytest.raises(rt.RtError, match="rt_set_lens"):
            lensed.set_lens(bad)
        assert np.array_equal(_bits(lensed.render(scene.camera, p)[0]), _bits(before)), bad
    lensed.set_lens((0.0, 0.0))  # a pinhole needs no plane of focus
    zero = lensed.render(scene.camera, p)[0]
    lensed.set_lens(None)
    assert np.array_equal(_bits(zero), _bits(lensed.render(scene.camera, p)[0])) and not np.array_equal(_bits(zero), _bits(before))
    m = rt.MultiRenderer([0, 0], copy_gather=True)
    try:
        m.upload(scene)
        m.set_lens((0.3, 4.0))
        with pytest.raises(rt.RtError, match="rt_set_lens"):
            m.set_lens((0.3, -1.0))
        img = m.render(scene.camera, p)[0]
        assert np.array_equal(_bits(img), _bits(before))
    finally:
        m.close()
