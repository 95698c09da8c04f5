"""Motion blur on the GPU (rt_set_motion).  Static frames do not move by one bit; the motion kernels with nothing displaced render the
static frame; a frozen shutter is the static scene at c(tm); single rays and whole images of black movers equal the numpy restatement
(tests/motion_ref.py) exactly; every search path agrees; the swept bounds are conservative; invalid motion is refused.

The float64 false-positive exception that the search-agreement tests of tests/test_gpu_parity.py allow is not used here: the frames
of the frozen-shutter and search-path tests are required to be equal outright (stricter)."""
import os
import sys

import numpy as np
import pytest

import lens_ref
import motion_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import np_ref  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def _bits(img):
    return img.view(np.uint32)


def _same(a, b, what=""):
    assert np.array_equal(_bits(a[0]), _bits(b[0])), what
    assert a[2].n_rays == b[2].n_rays and list(a[2].rays_per_depth) == list(b[2].rays_per_depth), what


def _centres(scene):
    a = scene.arrays()
    return np.stack([a["sph_cx"], a["sph_cy"], a["sph_cz"]], axis=1).astype(f32)


def _bare(scene):
    """indices of the spheres that may move: no wrapper, not a medium boundary, and no -0.0 centre component (c0 + 0 is +0.0)"""
    a = scene.arrays()
    n = scene.flat.n_spheres
    xf = a["sph_xform"] if len(a["sph_xform"]) else np.full(n, 0xFFFFFFFF, np.uint32)
    med = a["sph_medium"] if len(a["sph_medium"]) else np.full(n, 0xFFFFFFFF, np.uint32)
    c = _centres(scene)
    neg_zero = ((c == 0) & np.signbit(c)).any(axis=1)
    return np.nonzero((xf == 0xFFFFFFFF) & (med == 0xFFFFFFFF) & ~neg_zero)[0].astype(np.uint32)


@pytest.fixture
def fresh(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


SCENES = [("sphere_scene", 160, 90, 8, 12, (0.05, 10.0)), ("cornell_box", 96, 96, 8, 12, (10.0, 800.0)),
          ("final_scene", 96, 96, 6, 8, (10.0, 630.0))]


# ---- 3. static frames do not move ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nx,ny,spp,depth,lens", SCENES)
def test_static_frames_do_not_move(rt, fresh, name, nx, ny, spp, depth, lens):
    scene = rt.Scene.build(name, nx / ny)
    fresh.upload(scene)
    idx = _bare(scene)
    c1 = _centres(scene)[idx] + f32(0.25)
    p = rt.make_params(nx, ny, spp, max_depth=depth, seed=7)
    info = fresh.scene_info()
    for ln in (None, lens):
        fresh.set_lens(ln)
        never = fresh.render(scene.camera, p)
        fresh.set_motion(None)
        _same(never, fresh.render(scene.camera, p), (name, "NULL"))
        fresh.set_motion(rt.make_motion(idx, c1))
        moved = fresh.render(scene.camera, p)
        assert len(idx) == 0 or not np.array_equal(_bits(moved[0]), _bits(never[0]))  # (cornell_box has no sphere to move)
        fresh.set_motion(rt.make_motion([], np.zeros((0, 3)), (0.2, 0.4)))  # n_moving 0 clears too
        _same(never, fresh.render(scene.camera, p), (name, "set then clear"))
        assert fresh.scene_info() == info  # the search structures of the upload are back
    fresh.set_motion(rt.make_motion(idx, c1))
    fresh.upload(scene)  # an upload clears the motion
    fresh.set_lens(None)
    _same(fresh.render(scene.camera, p), rt_static(rt, scene, p), (name, "upload clears"))


def rt_static(rt, scene, p, lens=None, flags=None):
    r = rt.Renderer(0)
    try:
        r.upload(scene)
        r.set_lens(lens)
        return r.render(scene.camera, p)
    finally:
        r.close()


# ---- 4. the motion kernels with nothing displaced -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nx,ny,spp,depth,lens", [SCENES[0], ("simple_light_scene", 96, 64, 8, 12, (0.2, 20.0)), SCENES[2]])
def test_motion_kernels_with_nothing_displaced_render_the_static_frame(rt, orc, fresh, name, nx, ny, spp, depth, lens):
    """n_moving > 0 with c1 == c0 runs every MOTION instantiation the scene selects (candidate lists, grid walk, general tree,
    shading) on centres c0 + tm * 0 = c0 (cornell_box has no sphere; simple_light_scene stands in as the small general scene): the frame passes
    the suite's check against the oracle, and equals the static renderer's frame and ray counts per depth bit for bit."""
    from test_gpu_parity import _compare_frames, _oracle, _rays_agree  # (the suite's frame check: _explain_outliers inside)
    scene = rt.Scene.build(name, nx / ny)
    fresh.upload(scene)
    idx = _bare(scene)
    assert len(idx) > 0
    c0 = _centres(scene)[idx]
    # the motion frame itself against the oracle (which knows no motion, and needs none here): RMSE <= 2e-5 display units, no pixel
    # off by more than 1e-4 unless re-traced and explained, ray counts per depth exact (to 1e-4 with media)
    p = rt.make_params(nx, ny, spp, max_depth=depth, seed=7)
    fresh.set_motion(rt.make_motion(idx, c0, (0.0, 1.0)))
    img, _, st = fresh.render(scene.camera, p)
    ref, _, so = _oracle(orc, scene, p)
    _rays_agree(st, so, scene, p)
    _compare_frames(orc, scene, p, img, ref, name + " through the motion kernels", rt, fresh)
    for ln in (None, lens):
        fresh.set_lens(ln)
        for flags in (0, rt._ffi.FLAG_BRUTE_FORCE):
            p = rt.make_params(nx, ny, spp, max_depth=depth, seed=7, flags=flags)
            fresh.set_motion(None)
            static = fresh.render(scene.camera, p)
            fresh.set_motion(rt.make_motion(idx, c0, (0.0, 1.0)))
            _same(static, fresh.render(scene.camera, p), (name, ln, flags))


# ---- 5. a frozen shutter is a static scene ----------------------------------------------------------------------------------------
def _random_scene(rt, seed, n, with_rect, at=None):
    """n small spheres over a ground sphere; `at` replaces the centres (the static scene of a frozen shutter)"""
    f = rt._ffi
    rng = np.random.default_rng(seed)
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    cols = [tuple(float(x) for x in rng.uniform(0.2, 0.9, 3)) for _ in range(4)]
    mats = [s.material(f.MAT_DIFFUSE, tex0=s.constant_tex(c)) for c in cols]
    mats.append(s.material(f.MAT_METAL, color=(0.8, 0.7, 0.6), p=(0.1,)))
    _random_scene.mat_of = lambda k: ({"type": 1, "tex": cols[k % 5]} if k % 5 < 4 else {"type": 3, "color": (0.8, 0.7, 0.6), "p0": 0.1})  # np_ref.scatter
    c0 = np.concatenate([[[0.0, -1000.0, 0.0]], np.stack([rng.uniform(-8, 8, n), rng.uniform(0.2, 0.6, n), rng.uniform(-8, 8, n)], axis=1)]).astype(f32)
    c1 = (c0 + np.concatenate([[[0, 0, 0]], rng.uniform(-0.4, 0.4, (n, 3))])).astype(f32)
    rad = np.concatenate([[1000.0], np.full(n, 0.2)]).astype(f32)
    cc = c0 if at is None else at
    for k in range(n + 1):
        s.sphere(tuple(float(x) for x in cc[k]), float(rad[k]), mats[k % len(mats)], "s%d" % k)
    if with_rect:
        s.rect(f.RECT_XZ, (-3, 1.5, -3), (3, 1.5, 3), mats[0])
    s.set_camera((13, 3, 4), (0, 0.3, 0), (0, 1, 0), 25.0, 16 / 9)
    return s.finish(use_bvh=False), c0, c1


@pytest.mark.parametrize("seed,n,with_rect,want_grid", [(1, 40, False, False), (2, 60, True, False), (3, 600, False, True)])
@pytest.mark.parametrize("u0", [0.0, 0.37, 1.0])
def test_frozen_shutter_is_the_static_scene_at_that_time(rt, fresh, seed, n, with_rect, want_grid, u0):
    scene, c0, c1 = _random_scene(rt, seed, n, with_rect)
    idx = np.arange(1, n + 1, dtype=np.uint32)  # every small sphere moves; the ground stays
    at = c0.copy()
    at[idx] = motion_ref.center_at(c0[idx], c1[idx], np.full(n, u0, f32))
    frozen, _, _ = _random_scene(rt, seed, n, with_rect, at=at)
    for flags in (rt._ffi.FLAG_BRUTE_FORCE, 0):
        p = rt.make_params(160, 90, 6, max_depth=10, seed=3, flags=flags)
        fresh.upload(frozen)
        want = fresh.render(frozen.camera, p)
        fresh.upload(scene)
        fresh.set_motion(rt.make_motion(idx, c1[idx], (u0, u0)))
        if want_grid and not flags:
            assert fresh.scene_info()["grid"] == 1
        got = fresh.render(scene.camera, p)
        n_diff = int((_bits(got[0]) != _bits(want[0])).any(axis=2).sum())
        print("seed %d u0 %g flags %d: %d pixels differ" % (seed, u0, flags, n_diff))
        _same(want, got, (seed, u0, flags))


# ---- 6. single rays with a real shutter -------------------------------------------------------------------------------------------
def test_debug_bounce_hits_the_sphere_where_it_is_at_the_rays_time(rt, fresh):
    from helpers import path_keys
    scene, c0, c1 = _random_scene(rt, 11, 30, False)
    n = 30
    idx = np.arange(1, n + 1, dtype=np.uint32)
    shutter = (0.25, 0.75)
    fresh.upload(scene)
    fresh.set_motion(rt.make_motion(idx, c1[idx], shutter))
    rng = np.random.default_rng(4)
    m = 4096
    which = rng.integers(1, n + 1, m)
    keys = path_keys(0, np.arange(m), np.zeros(m, np.int64))  # (the production path derives slot i's key: seed 0, pixel i, sample 0)
    tm = motion_ref.path_time(keys, *shutter)
    assert tm.min() >= 0.25 and tm.max() <= 0.75 and tm.std() > 0.1
    target = np.where((np.arange(m) % 3 == 0)[:, None], c0[which], np.where((np.arange(m) % 3 == 1)[:, None], c1[which],
                      motion_ref.center_at(c0[which], c1[which], tm)))
    # towards an end position or the true one, grazing (offset by about a radius) every other ray, some from inside
    target = (target + rng.normal(size=(m, 3)) * np.where(np.arange(m) % 2 == 0, 0.2 / np.sqrt(3), 0.02)[:, None]).astype(f32)
    o = np.where((np.arange(m) % 7 == 0)[:, None], motion_ref.center_at(c0[which], c1[which], tm) + f32(0.05),
                 np.array([13, 3, 4], f32) + rng.normal(size=(m, 3))).astype(f32)
    d = (target - o).astype(np.float64)
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(f32)
    cen = np.tile(c0[None], (m, 1, 1))
    cen[:, idx] = np.stack([motion_ref.center_at(c0[i], c1[i], tm) for i in idx], axis=1)
    want_hit, want_t = np.full(m, -1), np.zeros(m, f32)
    want_alive, want_o, want_d, want_att = np.zeros(m, np.uint8), np.zeros((m, 3), f32), np.zeros((m, 3), f32), np.zeros((m, 3), f32)
    depth = 1
    for k in range(m):
        best, t_max = -1, f32(3.4028235e38)
        ok, dk = tuple(f32(x) for x in o[k]), tuple(f32(x) for x in d[k])
        for s in range(n + 1):  # HitableList::hit: t_max shrinks, a later equal root wins
            h = np_ref.sphere_hit(np_ref.v3(*cen[k, s]), f32(1000.0 if s == 0 else 0.2), ok, dk, f32(1e-3), t_max)
            if h is not None:
                best, t_max, rec = s, f32(h["t"]), h
        want_hit[k], want_t[k] = best, (t_max if best >= 0 else 0)
        if best >= 0:
            # the HitRecord of Sphere::hit on c(tm) — outward normal (p - c(tm)) / r — and the material's scatter with the path's key
            alive, att, so, sd, _ = np_ref.scatter(_random_scene.mat_of(best), dk, rec, np_ref.Rng(int(keys[k, 0]), int(keys[k, 1]), depth))
            if alive:
                want_alive[k], want_o[k], want_d[k], want_att[k] = 1, so, sd, att
    movers = want_hit > 0
    assert movers.mean() > 0.2
    assert (want_alive[movers & (want_hit % 5 < 4)] == 1).sum() > 200 and (want_alive[movers & (want_hit % 5 == 4)] == 1).sum() > 50  # Diffuse, Metal
    for flags in (0, rt._ffi.FLAG_BRUTE_FORCE, rt._ffi.FLAG_PRODUCTION_KERNELS, rt._ffi.FLAG_PRODUCTION_KERNELS | rt._ffi.FLAG_BRUTE_FORCE):
        out = fresh.debug_bounce(o, d, keys, depth=depth, flags=flags)
        assert np.array_equal(out["hit"], want_hit), (flags, int((out["hit"] != want_hit).sum()))
        assert np.array_equal(_bits(out["t"]), _bits(want_t)), flags
        assert np.array_equal(out["alive"], want_alive), (flags, int((out["alive"] != want_alive).sum()))
        for key, want in (("o", want_o), ("d", want_d), ("attenuation", want_att)):
            bad = (_bits(out[key]) != _bits(want)).any(axis=1) & (want_alive == 1)
            assert not bad.any(), (flags, key, int(bad.sum()), np.nonzero(bad)[0][:5], want_hit[bad][:5])


# ---- 7. the exact image of black movers -------------------------------------------------------------------------------------------
MOVERS = [((-1.5, 0.0, -4.0), (1.5, 0.3, -4.0), 0.6), ((0.6, -0.8, -2.5), (0.6, 0.7, -3.0), 0.3)]
CAM = ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 40.0, 1.5)


def _expected_black(scene, p, lens, shutter):
    jj, ii = np.meshgrid(np.arange(p.ny), np.arange(p.nx), indexing="ij")
    i, j = ii.ravel(), jj.ravel()
    acc = np.zeros((len(i), 3), f32)
    for s in range(p.spp):
        o, d, keys = lens_ref.lens_rays(scene.camera, p, i, j, np.full(len(i), s), lens[0], lens[1])
        tm = motion_ref.path_time(keys, *shutter)
        miss = np.ones(len(i), bool)
        for c0, c1, r in MOVERS:
            c = motion_ref.center_at(c0, c1, tm)
            for k in range(len(i)):
                if miss[k] and np_ref.sphere_hit(np_ref.v3(*c[k]), f32(r), tuple(o[k]), tuple(d[k]), f32(1e-3), f32(3.4028235e38)) is not None:
                    miss[k] = False
        acc = (acc + np.where(miss[:, None], lens_ref.sky_gradient(d), f32(0.0))).astype(f32)
    return (acc / f32(p.spp)).astype(f32).reshape(p.ny, p.nx, 3)


@pytest.mark.parametrize("lens", [(0.0, 1.0), (0.1, 3.5)])
@pytest.mark.parametrize("shutter", [(0.0, 1.0), (0.25, 0.5)])
def test_black_movers_image_is_the_restatement(rt, fresh, lens, shutter):
    """max_depth 0, black diffuse movers under the gradient sky: every pixel is the in-order f32 sum of sky(d) over the samples whose
    ray misses every mover where it is at the sample's time.  1 spp and 4 spp (candidate lists on): bit for bit (the 2 ulp once allowed
    with lists on had no cause in the code, and the largest difference measured on the MI355X is 0)."""
    f = rt._ffi
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    m = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.0, 0.0, 0.0)))
    for c0, c1, r in MOVERS:
        s.moving_sphere(c0, c1, r, m, "mover")
    s.set_camera(*CAM, shutter=shutter)
    scene = s.finish()
    fresh.upload(scene)
    fresh.set_lens(lens)
    fresh.set_motion(scene.motion)
    static = None
    for nx, ny, spp in ((48, 32, 1), (36, 24, 4)):
        p = rt.make_params(nx, ny, spp, max_depth=0, seed=21)
        img, _, st = fresh.render(scene.camera, p)
        want = _expected_black(scene, p, lens, shutter)
        hit = (want == 0).all(axis=2)
        assert 0.002 < hit.mean() < 0.9  # (blurred: few pixels are black in every sample)
        ulp = np.abs(img.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
        print("lens %r, shutter %r, %d spp: the largest difference is %d ulp" % (lens, shutter, spp, ulp))
        assert ulp == 0, (lens, shutter, spp, ulp)
        fresh.set_motion(None)
        static = fresh.render(scene.camera, p)[0]
        fresh.set_motion(scene.motion)
        assert not np.array_equal(_bits(static), _bits(img))  # the blur is there


def _edge_10_90(q):
    """(10 %-90 % width, 50 % point), in pixels, of a transmission profile that falls from 1 (sky) to 0 (sphere): first crossings,
    linear between pixel centres — the measure of tests/test_defocus.py"""
    def cross(level):
        k = int(np.argmax(q < level))
        assert k > 0
        return (k - 1) + (q[k - 1] - level) / (q[k - 1] - q[k])
    return cross(0.1) - cross(0.9), cross(0.5)


@pytest.mark.parametrize("shutter", [(0.0, 1.0), (0.25, 0.5)])
def test_streak_has_the_width_of_the_displacement_in_the_shutter(rt, fresh, shutter):
    """A black sphere crossing the view from c0 to c1 (along x, in the plane of the centre row) under the sky, max_depth 0, 1024 spp.
    Times are uniform over the shutter, so while it is open the silhouette's edge sweeps the image from where it is at `open` to where
    it is at `close`, and the transmission along the motion falls from 1 to 0 as a linear ramp of that length L (pixels): its 10-90 %
    width is 0.8 L, against the sharp (< 2 pixel) edge of the static sphere.  L is |c1 - c0| (close - open) projected — through the exact silhouette
    of a sphere seen in perspective, edge(x) = f tan(atan(x / z) +- asin(r / sqrt(x^2 + z^2))) — so the streak's 10 % extent exceeds the
    static sphere's by 0.8 L on either side, and with the shutter (0, 1) L is the whole projected displacement.  Asserted to one pixel:
    the width of each edge against 0.8 L and against the measured static edge swept along the motion, and the 50 % points of both edges against those of the static sphere
    standing where the mover is at mid shutter (extent and place of the streak)."""
    f = rt._ffi
    nx, ny, spp, vfov = 240, 100, 1024, 40.0
    c0, c1, r, z = np.array([-0.6, 0.0, -4.0]), np.array([0.6, 0.0, -4.0]), 0.8, 4.0
    cam = ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), vfov, nx / ny)
    px = ny / (2.0 * np.tan(np.radians(vfov) / 2.0))  # pixels per unit of the image plane at distance 1

    def scene_of(a, b):
        s = rt.Scene.new()
        s.set_sky(f.SKY_GRADIENT)
        m = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.0, 0.0, 0.0)))
        s.moving_sphere(tuple(float(x) for x in a), tuple(float(x) for x in b), r, m, "mover")
        s.set_camera(*cam, shutter=shutter)
        return s.finish()

    def edge(x, side):  # image column of the silhouette's left (-1) / right (+1) edge of the sphere centred at (x, 0, -z)
        return nx / 2.0 + px * np.tan(np.arctan(x / z) + side * np.arcsin(r / np.hypot(x, z)))
    p = rt.make_params(nx, ny, spp, max_depth=0, seed=5)
    rows = slice(ny // 2 - 1, ny // 2 + 1)  # the two rows next to the centre line

    def profile(scene, motion):
        fresh.upload(scene)
        fresh.set_motion(motion)
        return fresh.render(scene.camera, p)[0][rows, :, 0].mean(axis=0)
    behind = scene_of((0.0, 0.0, 9.0), (0.0, 0.0, 9.0))
    S = profile(behind, None)  # sky only
    mid_t = 0.5 * (shutter[0] + shutter[1])

    def x_of(t):
        return c0[0] + t * (c1[0] - c0[0])
    mover = scene_of(c0, c1)
    q_move = profile(mover, mover.motion) / S
    c_mid = c0 + mid_t * (c1 - c0)
    still = scene_of(c_mid, c_mid)  # the static sphere where the mover is at mid shutter
    q_still = profile(still, None) / S
    assert q_move.min() < 0.01 and q_still.min() < 0.01  # a fully covered core: the two ramps do not meet
    centre_col = int(0.5 * (edge(x_of(mid_t), +1) + edge(x_of(mid_t), -1)))
    ext = {}
    for name, q in (("move", q_move), ("still", q_still)):
        wl, ml = _edge_10_90(q[:centre_col + 1])                # left edge, scanned from the left
        wr, mr = _edge_10_90(q[::-1][:nx - centre_col])         # right edge, scanned from the right
        ext[name] = (wl, wr, ml, (nx - 1) - mr)
    for side, k in ((-1, 0), (+1, 1)):
        L = abs(edge(x_of(shutter[1]), side) - edge(x_of(shutter[0]), side))
        flat = px * np.linalg.norm(c1 - c0) * (shutter[1] - shutter[0]) / z  # |c1 - c0| in the shutter, projected without perspective
        assert abs(L - flat) < 0.05 * flat + 0.5
        print("shutter %s side %+d: edge width %.2f px, static %.2f px, ramp L %.2f px" % (shutter, side, ext["move"][k], ext["still"][k], L))
        # the streak is the time average of the static profile carried along by the edge: predicted from the measured static profile
        cols = np.arange(nx, dtype=np.float64)
        shifts = np.array([edge(x_of(t), side) - edge(x_of(mid_t), side) for t in np.linspace(shutter[0], shutter[1], 401)])
        pred = np.mean([np.interp(cols - sh, cols, q_still) for sh in shifts], axis=0)
        w_pred = _edge_10_90(pred[:centre_col + 1] if side < 0 else pred[::-1][:nx - centre_col])[0]
        assert abs(ext["move"][k] - w_pred) <= 1.0, (shutter, side, ext, w_pred)
        # and in closed form: a ramp of length L has the 10-90 % width 0.8 L; the static edge (a pixel's footprint and the silhouette's
        # curvature over two rows, under 2 pixels) is sharp against it, and two blurs do not add up linearly, so it stays within the pixel
        assert ext["still"][k] < 2.0 and abs(ext["move"][k] - 0.8 * L) <= 1.0, (shutter, side, ext, L)
    assert abs(ext["move"][2] - ext["still"][2]) <= 1.0 and abs(ext["move"][3] - ext["still"][3]) <= 1.0, ext


# ---- 8. every search path agrees: a general scene with movers -----------------------------------------------------------------------
def _general_scene(rt, seed=17, n=60):
    """spheres over a ground sphere, a rectangle, a box below RotateY + Translate, a fog box and a fog sphere — the bare small
    spheres move; returns (scene, motion)"""
    f = rt._ffi
    rng = np.random.default_rng(seed)
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    mats = [s.material(f.MAT_DIFFUSE, tex0=s.constant_tex(tuple(float(x) for x in rng.uniform(0.2, 0.9, 3)))) for _ in range(3)]
    mats.append(s.material(f.MAT_METAL, color=(0.8, 0.7, 0.6), p=(0.05,)))
    mats.append(s.material(f.MAT_DIELECTRIC, p=(1.5,)))
    white = mats[0]
    s.sphere((0.0, -1000.0, 0.0), 1000.0, mats[1], "ground")
    c0 = np.stack([rng.uniform(-6, 6, n), rng.uniform(0.2, 0.5, n), rng.uniform(-6, 6, n)], axis=1).astype(f32)
    c1 = (c0 + rng.uniform(-0.5, 0.5, (n, 3)) * np.array([1, 0.6, 1])).astype(f32)
    c1[:, 1] = np.maximum(c1[:, 1], f32(0.2))
    for k in range(n):
        s.moving_sphere(tuple(float(x) for x in c0[k]), tuple(float(x) for x in c1[k]), 0.2, mats[k % 5], "m%d" % k)
    s.rect(f.RECT_XZ, (-2.0, 1.6, -2.0), (2.0, 1.6, 2.0), white)
    s.translate(s.rotate_y(s.gbox((0.0, 0.0, 0.0), (1.0, 1.4, 1.0), white), 20.0), (2.5, 0.0, -1.0))
    fog = s.constant_tex((0.9, 0.9, 0.9))
    s.constant_medium(s.gbox((-3.5, 0.0, 0.5), (-2.0, 1.2, 2.0), white), 0.8, fog)
    s.constant_medium(s.sphere((0.0, 0.8, 3.0), 0.7, white, "fog ball"), 0.6, fog)
    s.set_camera((13, 4, 5), (0, 0.4, 0), (0, 1, 0), 25.0, 16 / 9, shutter=(0.1, 0.9))
    scene = s.finish()
    return scene, scene.motion


def test_every_search_path_agrees_on_a_general_scene_with_movers(rt, fresh):
    """The general MOTION instantiations (rectangles, wrappers, media; tables in LDS or not; tree in LDS and through L2) with real
    displacements and a real shutter — every ray its own time, recomputed from its slot past depth 0 — against the list walk, across
    options, slices and shards, and on two contexts."""
    from ray_tracing_in_one_weekend_amd import shard
    nx, ny = 128, 72
    scene, motion = _general_scene(rt)
    assert motion.n_moving == 60 and scene.flat.n_rects > 0 and scene.flat.n_xforms > 0 and scene.flat.n_media == 2
    fresh.upload(scene)
    p = rt.make_params(nx, ny, 6, max_depth=8, seed=11)
    static = fresh.render(scene.camera, p)
    for lens in (None, (0.05, 14.0)):
        fresh.set_lens(lens)
        ref = None
        for placement in (0, 1):  # tree in LDS / through L2 (read at upload and at set_motion)
            for tables in (0, 1):  # wrapper and medium tables in LDS / in HBM
                fresh.set_option("tree_placement", placement)
                fresh.set_option("general_lds", tables)
                fresh.upload(scene)
                fresh.set_motion(motion)
                info = fresh.scene_info()
                assert info["general_kernels"] == 1 and info["tree_in_lds"] == 1 - placement
                got = fresh.render(scene.camera, p)
                if ref is None:
                    ref = got
                    assert not np.array_equal(_bits(ref[0]), _bits(static[0]))
                    _same(ref, fresh.render(scene.camera, rt.make_params(nx, ny, 6, max_depth=8, seed=11, flags=rt._ffi.FLAG_BRUTE_FORCE)), "list walk")
                    for opt, val in (("primary_lists", 1), ("materialise_primaries", 1), ("pixel_order", 1)):
                        fresh.set_option(opt, val)
                        g2 = fresh.render(scene.camera, p)
                        fresh.set_option(opt, 0)
                        _same(ref, g2, (opt, val, lens))
                    _same(ref, fresh.render(scene.camera, rt.make_params(nx, ny, 6, max_depth=8, seed=11, spp_slice=2)), "3 slices")
                    parts = [fresh.render(scene.camera, rt.make_params(nx, ny, 6, max_depth=8, seed=11, shard_band=8, shard_count=4,
                                                                       shard_id=k))[0] for k in range(4)]
                    assert np.array_equal(_bits(shard.deinterleave(parts, ny, 8, 4)), _bits(ref[0]))
                else:
                    _same(ref, got, (lens, placement, tables))
        fresh.set_option("tree_placement", 0)
        fresh.set_option("general_lds", 0)
    fresh.upload(scene)
    fresh.set_lens(None)
    fresh.set_motion(motion)
    ref = fresh.render(scene.camera, p)
    m = rt.MultiRenderer([0, 0], copy_gather=True)
    try:
        m.upload(scene)
        m.set_motion(motion)
        img, _, st = m.render(scene.camera, p)
        assert np.array_equal(_bits(img), _bits(ref[0])) and st.n_rays == ref[2].n_rays
    finally:
        m.close()


# ---- 8b. every search path agrees: moving_sphere_scene -----------------------------------------------------------------------------------------------
def test_every_search_path_agrees_on_moving_sphere_scene(rt, fresh):
    from ray_tracing_in_one_weekend_amd import shard
    nx, ny = 128, 72
    scene = rt.Scene.build("moving_sphere_scene", nx / ny)
    fresh.upload(scene)
    p = rt.make_params(nx, ny, 6, max_depth=8, seed=11)
    static = fresh.render(scene.camera, p)
    for lens in (None, (0.05, 10.0)):
        fresh.set_lens(lens)
        fresh.set_motion(scene.motion)
        assert fresh.scene_info()["grid"] == 1
        ref = fresh.render(scene.camera, p)
        assert not np.array_equal(_bits(ref[0]), _bits(static[0]))
        _same(ref, fresh.render(scene.camera, rt.make_params(nx, ny, 6, max_depth=8, seed=11, flags=rt._ffi.FLAG_BRUTE_FORCE)), "list walk")
        for opt, val in (("grid", 1), ("primary_lists", 1), ("materialise_primaries", 1), ("pixel_order", 1)):
            fresh.set_option(opt, val)
            got = fresh.render(scene.camera, p)
            fresh.set_option(opt, 0)
            _same(ref, got, (opt, val, lens))
        _same(ref, fresh.render(scene.camera, rt.make_params(nx, ny, 6, max_depth=8, seed=11, spp_slice=2)), "3 slices")
        parts = [fresh.render(scene.camera, rt.make_params(nx, ny, 6, max_depth=8, seed=11, shard_band=8, shard_count=4, shard_id=k))[0]
                 for k in range(4)]
        assert np.array_equal(_bits(shard.deinterleave(parts, ny, 8, 4)), _bits(ref[0]))
    fresh.set_lens(None)
    fresh.set_option("tree_placement", 1)  # tree through L2 (read at upload / set_motion)
    fresh.upload(scene)
    fresh.set_motion(scene.motion)
    ref = fresh.render(scene.camera, p)
    fresh.set_option("tree_placement", 0)
    fresh.upload(scene)
    fresh.set_motion(scene.motion)
    _same(ref, fresh.render(scene.camera, p), "tree placement")
    m = rt.MultiRenderer([0, 0], copy_gather=True)
    try:
        m.upload(scene)
        m.set_motion(scene.motion)
        img, _, st = m.render(scene.camera, p)
        assert np.array_equal(_bits(img), _bits(ref[0])) and st.n_rays == ref[2].n_rays
    finally:
        m.close()


# ---- 9. the bounds are conservative -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["moving_sphere_scene", "random", "far"])
def test_motion_bounds_are_conservative(rt, fresh, which):
    if which == "moving_sphere_scene":
        scene = rt.Scene.build(which, 16 / 9)
        mo = scene.motion
        idx = np.array([mo.sphere[k] for k in range(mo.n_moving)], np.uint32)
        c1 = np.array([mo.center1[k] for k in range(3 * mo.n_moving)], f32).reshape(-1, 3)
        c0 = _centres(scene)
    else:
        scene, c0, c1a = _random_scene(rt, 3, 600, False)
        idx = np.arange(1, 601, dtype=np.uint32)
        c1 = c1a[idx]
        if which == "far":  # a few fast movers: "large" for the grid
            c1[:3] += f32(5.0)
    rad = scene.arrays()["sph_r"]
    fresh.upload(scene)
    fresh.set_motion(rt.make_motion(idx, c1))
    b = fresh.motion_bounds()
    entry_of = {int(e): k for k, e in enumerate(b["entry_id"])}
    rng = np.random.default_rng(9)
    pick = rng.integers(0, len(idx), 1000)
    tm = rng.uniform(0, 1, 1000).astype(f32)
    tm[:50], tm[50:100] = 0.0, 1.0
    c = np.stack([motion_ref.center_at(c0[idx[k]], c1[k], tm[t])[0] for t, k in enumerate(pick)]).astype(np.float64)
    has_grid = b["grid_dims"][0] > 0
    assert has_grid
    g0, cs, dims = b["grid_min"].astype(np.float64), b["grid_cell"].astype(np.float64), np.array(b["grid_dims"])
    for t, k in enumerate(pick):
        e = entry_of[int(idx[k])]
        r = float(rad[idx[k]])
        box = b["entry_box_padded"][e].astype(np.float64)
        assert np.all(c[t] - r >= box[:3]) and np.all(c[t] + r <= box[3:]), (which, k)
        bs = b["entry_sphere"][e].astype(np.float64)
        assert np.linalg.norm(c[t] - bs[:3]) + r <= bs[3], (which, k)
        cells = set(int(x) for x in b["cell_id"][b["cell_begin"][k]:b["cell_begin"][k + 1]])
        if cells == {0xFFFFFFFF}:
            continue  # tested for every ray
        lo = np.clip(np.floor((c[t] - r - g0) / cs), 0, dims - 1).astype(int)
        hi = np.clip(np.floor((c[t] + r - g0) / cs), 0, dims - 1).astype(int)
        for z in range(lo[2], hi[2] + 1):
            for y in range(lo[1], hi[1] + 1):
                for x in range(lo[0], hi[0] + 1):
                    assert (z * dims[1] + y) * dims[0] + x in cells, (which, k, x, y, z)


# ---- 10. validation ---------------------------------------------------------------------------------------------------------------
def test_invalid_motion_is_refused_and_the_previous_state_stays(rt, fresh):
    fin = rt.Scene.build("final_scene", 1.0)
    mk = rt.make_motion
    with pytest.raises(rt.RtError) as e:
        fresh.set_motion(mk([0], [[0, 0, 0]]))
    assert "(-5)" in str(e.value)  # RT_ERR_STATE: before upload
    fresh.upload(fin)
    bare = _bare(fin)
    a = fin.arrays()
    wrapped = np.nonzero(a["sph_xform"] != 0xFFFFFFFF)[0]
    medium = np.nonzero(a["sph_medium"] != 0xFFFFFFFF)[0]
    assert len(bare) >= 2 and len(wrapped) > 0 and len(medium) > 0
    c = _centres(fin)
    p = rt.make_params(64, 64, 4, max_depth=6, seed=2)
    good = mk(bare[:2], c[bare[:2]] + f32(20.0), (0.1, 0.9))
    fresh.set_motion(good)
    ref = fresh.render(fin.camera, p)
    n = fin.flat.n_spheres
    bad = [(mk([bare[1], bare[0]], c[bare[:2]]), -1), (mk([bare[0], bare[0]], c[bare[:2]]), -1), (mk([n], c[:1]), -1),
           (mk([int(wrapped[0])], c[:1]), -4), (mk([int(medium[0])], c[:1]), -4), (mk([bare[0]], [[np.nan, 0, 0]]), -1),
           (mk([bare[0]], c[:1], (0.6, 0.5)), -1), (mk([bare[0]], c[:1], (-0.1, 0.5)), -1), (mk([bare[0]], c[:1], (0.0, 1.1)), -1)]
    for motion, code in bad:
        with pytest.raises(rt.RtError) as e:
            fresh.set_motion(motion)
        assert "(%d)" % code in str(e.value), (e.value, code)
        _same(ref, fresh.render(fin.camera, p), "previous state kept")
    with pytest.raises(rt.RtError, match="bare"):
        fresh.set_motion(mk([int(wrapped[0])], c[:1]))
