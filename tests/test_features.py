"""The first-hit features on the GPU (rt_accum_track_features, rt_accum_read_features, rt_accum_export_features, rt_accum_import_features,
rt_debug_features_add) against tests/features_ref.py, which uses nothing of k_features: the records and the read-out bit for bit — the
normal, the depth, the counters and the f64 moments against the numpy restatement, the albedo against shade()'s own output or the scene
description (features_ref says which) —; the same bits however a window is cut and whichever search form finds the hits; every set and
scene kind; adaptive adds; resume; the refusals and errors of the header; and everything else an accumulation returns unchanged.  No
comparison here has a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

import features_ref as ref
import frame_cases as fc
from helpers import STATS_COUNTERS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
BRUTE = ref.FLAG_BRUTE_FORCE
SPP = 5
# nx, ny: a single pixel; partial 32 x 32 blocks on both axes with two blocks along x; the smallest tiled geometry of tests/frame_cases.py
# (tiles plus a 3-row tail)
SHAPES = {"1x1": (1, 1), "33x9": (33, 9), "16x11": (16, 11), "24x13": (24, 13), "40x20": (40, 20)}


def _raises(rt, code, fn, *a, **kw):
    with pytest.raises(rt.RtError, match=r"\(-%d\)" % code):
        fn(*a, **kw)


def _plane_is(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    for name in want.dtype.names:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        bits = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
        bad = g.view(bits) != w.view(bits)
        if bad.any():
            at = tuple(int(i) for i in np.argwhere(bad)[0])
            raise AssertionError((what, name, int(bad.sum()), "values differ, first at", at, g[at], w[at]))


def _read_is(r, want, what):
    got, exp = r.accum_features(), ref.read_out(want)
    for k in ("albedo", "normal", "depth", "hit", "var"):
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k)
        bad = got[k].view(np.uint32) != exp[k].view(np.uint32)
        assert not bad.any(), (what, k, int(bad.sum()), "values differ, first at", tuple(int(i) for i in np.argwhere(bad)[0]))


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    yield r
    r.set_option("tree_placement", 0)
    r.close()


# ---- scenes and their reference samples: made once, never changed ----------------------------------------------------------------------
_scenes, _hits = {}, {}


def _quads_arrays(q):
    arr = lambda p, n, dt: np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True)
    return (arr(q.q, 3 * q.n, f32).reshape(-1, 3), arr(q.u, 3 * q.n, f32).reshape(-1, 3), arr(q.v, 3 * q.n, f32).reshape(-1, 3),
            arr(q.kind, q.n, np.uint8), arr(q.mat, q.n, np.uint32))


def texture_scene(rt, aspect):
    """Every material tag and texture kind in front of the camera, one sphere each on a 5 x 4 lattice over a checkered rectangle: Diffuse
    over a constant, a checker, a Perlin and an image texture; Lambert, the pbr.rs family, Metal, Dielectric, DisneyClearcoat and an
    Emission brighter than 1 over constants; Translate(RotateY(..)) on a sphere and on a box; chains of six wrappers (more than RT_MAX_CHAIN)
    on a sphere and on a box; and a thin fog sphere, which depth-0 rays both scatter in and pass."""
    f = rt._ffi
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    const = lambda c: s.constant_tex(c)
    checker = s.checker_tex((0.1, 0.1, 0.8), (0.9, 0.9, 0.9))
    mats = [s.material(f.MAT_DIFFUSE, tex0=const((0.2, 0.9, 0.4))), s.material(f.MAT_DIFFUSE, tex0=checker),
            s.material(f.MAT_DIFFUSE, tex0=s.perlin_tex(4.0)), s.material(f.MAT_DIFFUSE, tex0=s.image_tex("res/earthmap.jpg")),
            s.material(f.MAT_LAMBERT, tex0=const((0.5, 0.7, 0.6))), s.material(f.MAT_METAL, color=(0.8, 0.7, 0.6), p=(0.3,)),
            s.material(f.MAT_DIELECTRIC, p=(1.5,)), s.material(f.MAT_EMISSION, tex0=const((4.0, 0.5, 3.0))),
            s.material(f.MAT_OREN_NAYAR, tex0=const((0.7, 0.3, 0.2)), p=(0.5,)), s.material(f.MAT_BURLEY_DIFFUSE, tex0=const((0.3, 0.6, 0.7)), p=(0.5,)),
            s.material(f.MAT_ROUGH_PLASTIC, tex0=const((0.9, 0.8, 0.1)), tex1=const((0.2, 0.2, 0.7)), p=(0.3, 1.5)),
            s.material(f.MAT_DISNEY_DIFFUSE, tex0=const((0.6, 0.1, 0.6)), p=(0.5, 0.5)), s.material(f.MAT_DISNEY_METAL, tex0=const((0.95, 0.6, 0.3)), p=(0.4, 0.2, 0.1)),
            s.material(f.MAT_DISNEY_SHEEN, tex0=const((0.4, 0.5, 0.9)), p=(0.5,)), s.material(f.MAT_DISNEY_CLEARCOAT, p=(0.5,))]
    at = lambda k: (-4.0 + 2.0 * (k % 5), 0.2 + 1.9 * (k // 5), 0.0)
    for k, m in enumerate(mats):
        s.sphere(at(k), 0.8, m, "m%d" % k)
    s.translate(s.rotate_y(s.sphere((0.0, 0.0, 0.0), 0.8, mats[1], "wrapped"), 30.0), at(15))
    h = s.sphere((0.0, 0.0, 0.0), 0.8, mats[2], "deep")
    for k in range(5):
        h = s.rotate_y(h, 10.0 + 7.0 * k) if k % 2 == 0 else s.translate(h, (0.05 * k, 0.0, -0.03 * k))
    s.translate(h, at(16))
    s.constant_medium(s.sphere(at(17), 0.8, mats[0], "fog"), 0.9, const((0.9, 0.5, 0.3)))
    s.translate(s.rotate_y(s.gbox((-0.6, -0.6, -0.6), (0.6, 0.6, 0.6), mats[1]), 25.0), at(18))
    h = s.gbox((-0.6, -0.6, -0.6), (0.6, 0.6, 0.6), mats[0])
    for k in range(5):
        h = s.rotate_y(h, -12.0 - 5.0 * k) if k % 2 == 0 else s.translate(h, (-0.04 * k, 0.02 * k, 0.0))
    s.translate(h, at(19))
    s.rect(f.RECT_XZ, (-7.0, -0.8, -4.0), (7.0, -0.8, 6.0), mats[1])
    s.set_camera((0.5, 3.2, 13.0), (0.0, 3.0, 0.0), (0, 1, 0), 36.0, aspect)
    return s.finish()


def _scene(rt, kind, shape):
    nx, ny = SHAPES[shape]
    key = (kind, shape)
    if key not in _scenes:
        _scenes[key] = {"spheres": lambda: fc.sphere_scene(rt, nx / ny), "general": lambda: (fc.general_scene(rt, nx / ny),),
                        "textures": lambda: (texture_scene(rt, nx / ny),)}[kind]()
    return _scenes[key]


class Case:
    """One scene under one set at one frame size: `apply` puts it on a context, `hits` are the reference samples 0 .. 5."""

    def __init__(self, rt, kind, shape, lens=None, motion=False, quads=False, lights=False):
        self.rt, self.kind, self.shape = rt, kind, shape
        self.nx, self.ny = SHAPES[shape]
        got = _scene(rt, kind, shape)
        self.scene = got[0]
        self.lens = lens
        self.motion = (got[1], got[2], fc.SHUTTER) if motion else None
        self.quads = _quads_arrays(self.scene.quads) if quads else None
        self.lights = lights
        self.key = (kind, shape, lens, motion, quads)  # (a light set changes no feature: not part of the key)

    def params(self, spp=SPP, **kw):
        return self.rt.make_params(self.nx, self.ny, spp, **{"max_depth": 5, "seed": 4711, **kw})

    def apply(self, r):
        r.upload(self.scene)
        r.set_lens(self.lens)
        r.set_motion(self.rt.make_motion(*self.motion) if self.motion else None)
        r.set_quads(self.scene.quads if self.quads else None)
        lights = None
        if self.lights:
            lights = self.rt.make_lights(*_scene(self.rt, self.kind, self.shape)[3]) if self.kind == "spheres" else self.scene.lights
        r.set_lights(lights)

    def hits(self, r):
        """feature samples 0 .. 5 of every pixel (the context holds the case, without its light set: the hook's Diffuse attenuation carries
        the light weight under one)"""
        if self.key not in _hits:
            fh = ref.first_hits(r, self.scene, self.params(), np.arange(SPP + 1), self.lens, self.motion, self.quads)
            for v in fh.values():
                v.setflags(write=False)
            _hits[self.key] = fh
        return _hits[self.key]


def _window(fh, first, n, stride):
    """the samples of `fh` (indices 0 .. 5) that the window first .. first + n - 1 contributes"""
    idx = ref.contributing(first, n, stride)
    return {k: v[idx] for k, v in fh.items()}


def _prepared(rt, r, *a, **kw):
    c = Case(rt, *a, **kw)
    lights, c.lights = c.lights, False
    c.apply(r)
    fh = c.hits(r)
    if lights:
        c.lights = True
        c.apply(r)
    return c, fh


# ---- 1. the defining property, and its independence of how a window is cut ---------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("shape", ["1x1", "33x9", "16x11"])
def test_records_are_the_in_order_sums_of_the_header_however_the_window_is_cut(rt, ctx, shape, stride):
    r = ctx
    c, fh = _prepared(rt, r, "spheres", shape)
    assert fh["hit"].any()  # (this scene's ground and ball leave the sky to few pixels: the misses are test 3's)
    for first in (0, 1):
        want = ref.accumulate(_window(fh, first, SPP, stride))
        # at once, through the add itself (slices of 2: the window is cut inside the add as well)
        r.accum_begin(c.scene.camera, c.params(spp_slice=2), first_sample=first)
        r.accum_track_features(stride)
        r.accum_add(SPP)
        snap = r.accum_export_features()
        assert (snap.nx, snap.rows, snap.first_sample, snap.done, snap.stride) == (c.nx, c.ny, first, SPP, stride) and snap.check()
        _plane_is(snap.plane, want, (shape, stride, first, "one add"))
        _read_is(r, want, (shape, stride, first, "one add"))
        # as 2 + 3, through two adds
        r.accum_begin(c.scene.camera, c.params(), first_sample=first)
        r.accum_track_features(stride)
        r.accum_add(2), r.accum_add(3)
        _plane_is(r.accum_export_features().plane, want, (shape, stride, first, "2 + 3"))
        # and through the hook alone, which traces nothing: 1 + 4
        r.accum_begin(c.scene.camera, c.params(), first_sample=first)
        r.accum_track_features(stride)
        r.debug_features_add(first, 1), r.debug_features_add(first + 1, 4)
        snap = r.accum_export_features()
        assert snap.done == 0
        _plane_is(snap.plane, want, (shape, stride, first, "hook 1 + 4"))
    # a window that holds no contributing sample changes nothing
    if stride == 3:
        r.debug_features_add(4, 2), r.debug_features_add(7, 2)
        _plane_is(r.accum_export_features().plane, want, (shape, stride, "empty windows"))
    r.accum_end()


# ---- 2. the three search forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spheres", "general"])
def test_the_three_search_forms_give_the_same_records(rt, ctx, kind):
    r = ctx
    quads = kind == "general"
    c, fh = _prepared(rt, r, kind, "24x13", quads=quads)
    want = ref.accumulate(_window(fh, 0, SPP, 1))
    planes = {}
    for form in ("lds", "l2", "brute"):
        r.set_option("tree_placement", 1 if form == "l2" else 0)
        c.apply(r)
        info = r.scene_info()
        if form == "lds" and kind == "spheres":
            assert info["tree_in_lds"]
        if form == "l2":
            assert not info["tree_in_lds"]
        r.accum_begin(c.scene.camera, c.params(flags=BRUTE if form == "brute" else 0))
        r.accum_track_features(1)
        r.accum_add(SPP) if form != "l2" else r.debug_features_add(0, SPP)
        planes[form] = r.accum_export_features().plane
        _plane_is(planes[form], want, (kind, form))
    r.accum_end()
    r.set_option("tree_placement", 0)


# ---- 3. sets and scene kinds ----------------------------------------------------------------------------------------------------------
SETS = {"lens": dict(kind="spheres", lens=fc.LENS_SPHERES), "motion": dict(kind="spheres", motion=True), "lights": dict(kind="spheres", lights=True),
        "quads": dict(kind="general", quads=True), "quads+lights+lens": dict(kind="general", quads=True, lights=True, lens=fc.LENS_GENERAL),
        "textures": dict(kind="textures")}


@pytest.mark.parametrize("name", list(SETS))
def test_records_under_every_set_and_scene_kind(rt, ctx, name):
    r = ctx
    kw = dict(SETS[name])
    kind = kw.pop("kind")
    c, fh = _prepared(rt, r, kind, "40x20" if kind == "textures" else "24x13", **kw)
    w = ref.World(c.scene, c.motion, c.quads)
    idx = fh["index"]
    tags = {int(w.a["mat_type"][w.material(int(h))]) for h in np.unique(idx[idx >= 0])}
    if name == "motion":
        moved = np.isin(idx, c.motion[0])
        assert moved.sum() >= 20, "moving spheres are hit"
    if "quads" in name:
        assert (idx >= w.pbase).sum() >= 20 and ((idx >= w.n_prims) & (idx < w.pbase)).any(), "planar primitives are hit and the medium scatters"
        chains = {len(ref._chain(w.a, w.a["rect_xform"][h - w.ns])) for h in np.unique(idx[(idx >= w.ns) & (idx < w.n_prims)])}
        assert 2 in chains, "the rotated and translated box is hit"
    if name == "textures":
        assert tags == set(range(13)), ("every material tag is hit", tags)
        depth = lambda h: len(ref._chain(w.a, w.a["sph_xform"][h] if h < w.ns else w.a["rect_xform"][h - w.ns]))
        hit_prims = [int(h) for h in np.unique(idx[(idx >= 0) & (idx < w.n_prims)])]
        assert {2, 6} <= {depth(h) for h in hit_prims if h < w.ns} and {2, 6} <= {depth(h) for h in hit_prims if h >= w.ns}, "short and deep chains, sphere and box"
        med = (idx >= w.n_prims) & (idx < w.pbase)
        assert med.sum() >= 10 and (fh["a"][med] == np.array([0.9, 0.5, 0.3], f32)).all(), "depth-0 rays scatter in the fog: its phase texture"
        assert (idx == 7).sum() >= 10 and (fh["a"][idx == 7] == np.array([1.0, 0.5, 1.0], f32)).all(), "the emitter's (4, 0.5, 3) is clamped"
    want = ref.accumulate(_window(fh, 0, SPP, 1))
    r.accum_begin(c.scene.camera, c.params(spp_slice=3))
    r.accum_track_features(1)
    r.accum_add(SPP)
    _plane_is(r.accum_export_features().plane, want, name)
    _read_is(r, want, name)
    r.accum_end()
    r.set_lens(None), r.set_motion(None), r.set_quads(None), r.set_lights(None)


def test_the_fog_sphere_is_both_scattered_in_and_passed(rt, ctx):
    r = ctx
    c, fh = _prepared(rt, r, "textures", "40x20")
    w = ref.World(c.scene)
    idx = fh["index"]
    scattered = (idx >= w.n_prims).any(axis=0)
    passed = (idx < w.n_prims).any(axis=0)
    assert (scattered & passed).sum() >= 3, "pixels whose samples both scatter in the medium and pass through it"
    assert np.all(fh["n"][idx >= w.n_prims] == 0)


# ---- 4. adaptive adds -----------------------------------------------------------------------------------------------------------------
def test_converged_pixels_take_no_feature_sample(rt, ctx):
    r = ctx
    c, fh = _prepared(rt, r, "spheres", "24x13")
    r.accum_begin(c.scene.camera, c.params())
    r.accum_track_features(1)
    r.accum_add(4)
    # a tolerance that about half of the pixels meet: the median of sem / max(Y, floor) after these four samples
    img, _, sem, _ = r.accum_read(want_sem=True)
    rel = sem / np.maximum(0.2126 * img[..., 0] + 0.7152 * img[..., 1] + 0.0722 * img[..., 2], 0.01)
    r.accum_add_adaptive(2, tolerance=float(np.median(rel)), min_samples=2)
    counts, _ = r.accum_counts()
    active = counts == 6
    assert active.any() and (~active).any() and set(np.unique(counts)) == {4, 6}, "some pixels converged, some went on"
    want = ref.accumulate(_window(fh, 0, 4, 1))
    want = ref.accumulate(_window(fh, 4, 2, 1), want, active)
    got = r.accum_export_features().plane
    _plane_is(got, want, "after an adaptive add")
    assert (got["n_f"] == counts).all()
    _read_is(r, want, "after an adaptive add")
    r.accum_end()


# ---- 5. resume, refusals and errors -----------------------------------------------------------------------------------------------------
def test_export_import_continue_and_what_is_refused(rt, ctx, tmp_path):
    r = ctx
    f = rt._ffi
    c, fh = _prepared(rt, r, "spheres", "24x13")
    cam = c.scene.camera
    _raises(rt, f.ERR_STATE, r.accum_track_features, 1)  # no open accumulation
    r.accum_begin(cam, c.params())
    _raises(rt, f.ERR_STATE, r.accum_features)            # not tracked
    _raises(rt, f.ERR_STATE, r.accum_export_features)
    _raises(rt, f.ERR_STATE, r.debug_features_add, 0, 1)
    for bad in (0, 65):
        _raises(rt, f.ERR_INVALID, r.accum_track_features, bad)
        assert not rt.features_check(bad)
    assert rt.features_check(1) and rt.features_check(64)
    r.accum_track_features(2)
    r.accum_track_features(2)                             # the same stride again: nothing changes
    _raises(rt, f.ERR_STATE, r.accum_track_features, 3)   # another one
    _raises(rt, f.ERR_INVALID, r.debug_features_add, 0, 0)
    _raises(rt, f.ERR_INVALID, r.debug_features_add, 0xFFFFFFFF, 2)
    r.accum_add(3)
    state, snap = r.accum_export(), r.accum_export_features()
    _raises(rt, f.ERR_UNSUPPORTED, r.accum_merge, state)
    _raises(rt, f.ERR_UNSUPPORTED, r.accum_import, state)
    r.accum_add(2)
    whole = r.accum_export_features().plane
    _plane_is(whole, ref.accumulate(_window(fh, 0, SPP, 2)), "uninterrupted")
    # through a file, into a fresh accumulation, then on
    snap.save(str(tmp_path / "features.npz"))
    back = rt.AccumFeatures.load(str(tmp_path / "features.npz"))
    assert back.check() and back.stride == 2 and ref.same_bits(back.plane, snap.plane)
    r.accum_begin(cam, c.params())
    r.accum_import(state)
    other = rt.AccumFeatures(back.nx, back.rows, back.first_sample, back.done + 1, back.frame_id, 2, back.plane)
    _raises(rt, f.ERR_INVALID, r.accum_import_features, other)
    r.accum_import_features(back)
    _raises(rt, f.ERR_STATE, r.accum_track_features, 3)
    r.accum_add(2)
    _plane_is(r.accum_export_features().plane, whole, "resumed")
    _raises(rt, f.ERR_STATE, r.accum_import_features, back)  # samples were added
    # tracking after samples
    r.accum_begin(cam, c.params())
    r.accum_add(1)
    _raises(rt, f.ERR_STATE, r.accum_track_features, 1)
    # a shard
    r.accum_begin(cam, c.params(shard_band=1, shard_count=2, shard_id=1))
    _raises(rt, f.ERR_UNSUPPORTED, r.accum_track_features, 1)
    r.accum_end()


def test_multi_accum_begin_refuses_the_features_bit(rt):
    """rt_multi_accum_begin with RT_MULTI_UNSUPPORTED_FEATURES, alone or beside a bit it covers: RT_ERR_UNSUPPORTED with a message, nothing begun;
    a bit that is no RT_MULTI_TRACK_* stays RT_ERR_INVALID; and the contexts go on as before."""
    import ctypes as C
    f = rt._ffi
    assert f.MULTI_UNSUPPORTED_FEATURES == 32
    c = Case(rt, "spheres", "24x13")
    m = rt.MultiRenderer([0, 0], copy_gather=True)
    try:
        m.upload(c.scene)
        cam, prm = c.scene.camera, c.params()
        for track in (f.MULTI_UNSUPPORTED_FEATURES, f.MULTI_UNSUPPORTED_FEATURES | f.MULTI_TRACK_CHANNELS, f.MULTI_UNSUPPORTED_FEATURES | f.MULTI_TRACK_BUCKETS):
            assert m._lib.rt_multi_accum_begin(m._m, C.byref(cam), C.byref(prm), 0, track, 5) == -f.ERR_UNSUPPORTED, track
            _raises(rt, f.ERR_STATE, m.accum_join)  # nothing was begun
        with pytest.raises(rt.RtError, match="RT_MULTI_UNSUPPORTED_FEATURES"):
            m._call("rt_multi_accum_begin", C.byref(cam), C.byref(prm), 0, f.MULTI_UNSUPPORTED_FEATURES, 0)
        assert m._lib.rt_multi_accum_begin(m._m, C.byref(cam), C.byref(prm), 0, 8, 0) == -f.ERR_INVALID
        m.accum_begin(cam, prm, channels=True)
        m.accum_add(2)
        j = m.accum_join()
        _raises(rt, f.ERR_STATE, j.accum_track_features, 1)  # the joined context: as every rt_accum_track_*
        _raises(rt, f.ERR_STATE, j.accum_features)
        m.accum_end()
    finally:
        m.close()


# ---- 6. an accumulation that tracks no features, and one that does, return what they returned ----------------------------------------------
def test_everything_else_an_accumulation_returns_is_unchanged(rt, ctx):
    r = ctx
    c, _ = _prepared(rt, r, "spheres", "24x13")
    fresh = rt.Renderer(0)  # a context that never heard of features
    try:
        c.apply(fresh)
        outs = []
        for ren, track in ((fresh, False), (r, False), (r, True)):
            ren.accum_begin(c.scene.camera, c.params(spp_slice=2))
            if track:
                ren.accum_track_features(2)
            st = ren.accum_add(SPP)
            img, rgb8, sem, noise = ren.accum_read(want_rgb8=True, want_sem=True)
            outs.append((img, rgb8, sem, ren.accum_export(), st))
            ren.accum_end()
        for img, rgb8, sem, state, st in outs[1:]:
            assert ref.same_bits(img, outs[0][0]) and ref.same_bits(rgb8, outs[0][1]) and ref.same_bits(sem, outs[0][2])
            assert ref.same_bits(state.sum, outs[0][3].sum) and ref.same_bits(state.moments, outs[0][3].moments)
            for k in STATS_COUNTERS:
                assert getattr(st, k) == getattr(outs[0][4], k), k
            assert list(st.rays_per_depth) == list(outs[0][4].rays_per_depth)
    finally:
        fresh.close()


# ---- 7. render.py -------------------------------------------------------------------------------------------------------------------------
def _render_py(*args):
    cmd = [sys.executable, "-m", "ray_tracing_in_one_weekend_amd.render", "--scene", "cornell_box", "--nx", "40", "--ny", "20", "--max-depth", "8",
           "--seed", "7", *[str(a) for a in args]]
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_render_py_writes_the_feature_images_and_resumes_the_records(rt, tmp_path):
    from ray_tracing_in_one_weekend_amd.images import read_pfm
    ck, ck2, ck3 = (tmp_path / n for n in ("ck.npz", "ck2.npz", "ck3.npz"))
    a, n, z = (tmp_path / k for k in ("a.pfm", "n.pfm", "z.pfm"))
    p = _render_py("--spp", 4, "--spp-step", 4, "--features", "--feature-stride", 2, "--checkpoint", ck, "--out", tmp_path / "part.png")
    assert p.returncode == 0, p.stderr[-2000:]
    snap = rt.AccumFeatures.load(str(ck) + ".features.npz")
    assert (snap.first_sample, snap.done, snap.stride) == (0, 4, 2) and snap.check() and (snap.plane["n_f"] == 2).all()
    p = _render_py("--spp", 6, "--spp-step", 4, "--features", "--feature-stride", 2, "--resume", ck, "--checkpoint", ck2, "--albedo-out", a, "--normal-out", n,
                   "--depth-out", z, "--out", tmp_path / "resumed.png")
    assert p.returncode == 0, p.stderr[-2000:]
    p = _render_py("--spp", 6, "--spp-step", 6, "--features", "--feature-stride", 2, "--checkpoint", ck3, "--out", tmp_path / "whole.png")
    assert p.returncode == 0, p.stderr[-2000:]
    resumed, whole = rt.AccumFeatures.load(str(ck2) + ".features.npz"), rt.AccumFeatures.load(str(ck3) + ".features.npz")
    assert ref.same_bits(resumed.plane, whole.plane) and (whole.plane["n_f"] == 3).all()
    out = ref.read_out(whole.plane)
    assert ref.same_bits(read_pfm(str(a)), out["albedo"]) and ref.same_bits(read_pfm(str(n)), out["normal"])
    assert ref.same_bits(read_pfm(str(z)), np.repeat(out["depth"][..., None], 3, axis=2))
    assert open(tmp_path / "resumed.png", "rb").read() == open(tmp_path / "whole.png", "rb").read()
    # what the command line refuses before it renders
    for bad in (("--features", "--feature-stride", 65), ("--albedo-out", a), ("--features", "--resume", ck, "--feature-stride", 3)):
        p = _render_py("--spp", 4, *bad, "--out", tmp_path / "bad.png")
        assert p.returncode == 2 and not os.path.exists(tmp_path / "bad.png"), (bad, p.stderr[-500:])
