"""The multi-scale filter on the GPU (rt_accum_denoise_multiscale, rt_debug_denoise_multiscale): the kernels of csrc/rt_multiscale.h and the
accumulation path against tests/denoise_multiscale_ref.py bit for bit, the filter's inputs of every level included; one level against the
two single-scale calls; the accumulation left undisturbed; the errors of the header; and the error of rendered frames against the
single-scale filter's."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref
import denoise_channels_ref as ch_ref
import denoise_multiscale_ref as ref
import denoise_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 1234
K = denoise_ref.KERNEL_CASE_STRENGTH
GUIDES = ["luminance", "channels"]
FRAMES = {
    "A": dict(scene="test_sphere", nx=40, ny=20, kw=dict(max_depth=50)),  # 40 x 20 -> 20 x 10 -> 10 x 5 -> 5 x 3
    "B": dict(scene="cornell_box", nx=23, ny=15, kw=dict(max_depth=8)),   # odd sides on every level: 23 x 15 -> 12 x 8 -> 6 x 4 -> 3 x 2
}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()), "values differ")


def _raises(rt, code, fn, *a, **kw):
    with pytest.raises(rt.RtError, match=r"\(-%d\)" % code):
        fn(*a, **kw)


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


_scenes, _single, _wanted = {}, {}, {}


def _setup(rt, r, case):
    c = FRAMES[case]
    if c["scene"] not in _scenes:
        _scenes[c["scene"]] = rt.Scene.build(c["scene"], c["nx"] / c["ny"])
    scene = _scenes[c["scene"]]
    r.upload(scene)
    return scene, lambda spp, **kw: rt.make_params(c["nx"], c["ny"], spp, seed=SEED, **{"spp_slice": 3, **c["kw"], **kw})


def _singles(r, scene, prm, case, n):
    """x[s], s < n: the single-sample frames of the case (first_sample = s, one add of 1), computed once and never changed."""
    have = _single.setdefault(case, [])
    for s in range(len(have), n):
        r.accum_begin(scene.camera, prm(1), first_sample=s)
        r.accum_add(1)
        img = r.accum_read()[0]
        img.setflags(write=False)
        have.append(img)
    r.accum_end()
    return have[:n]


# ---- 1. the kernels against the reference, through the debug call ---------------------------------------------------------------------
# 37 x 21 and 13 x 9 (R 10, F 3: the window is larger than every coarse level); 1 x 1; 2 x 2, whose coarse level is 1 x 1; a single row
# and a single column, k = 1 and 2; 17 x 33 and 33 x 17; 35 x 19 with odd sides at two levels and a coarse level of 18 x 10 across the
# 16-pixel tile of the filter.
KERNEL_CASES = [(37, 21, 5, 1), (37, 21, 1, 0), (13, 9, 10, 3), (1, 1, 5, 1), (2, 2, 5, 1), (3, 1, 2, 1), (1, 5, 2, 0), (17, 33, 2, 3), (33, 17, 10, 3),
                (35, 19, 3, 2)]


def _kernel_case(guide, nx, rows):
    """(c, mean or None, var) of the guide's kernel_case: with the NaN, the +inf and the zero-variance pixels."""
    if guide == "luminance":
        return denoise_ref.kernel_case(nx, rows)
    c, var = ch_ref.kernel_case(nx, rows)
    return c, None, var


def _reference(guide, c, mean, var, radius, patch, k, levels):
    """(o_0, levels) of the reference, computed once per argument set and shared."""
    key = (guide, c.shape, radius, patch, float(k), levels, _bits(c).tobytes()[:64])
    if key not in _wanted:
        _wanted[key] = ref.luminance(c, mean, var, radius, patch, k, levels) if guide == "luminance" else ref.channels(c, var, radius, patch, k, levels)
    return _wanted[key]


@pytest.mark.parametrize("levels", [2, 3, 4])
@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("nx,rows,radius,patch", KERNEL_CASES)
def test_kernels_match_the_reference_bit_for_bit(ctx, nx, rows, radius, patch, guide, levels):
    c, mean, var = _kernel_case(guide, nx, rows)
    want, lv = _reference(guide, c, mean, var, radius, patch, K, levels)
    one = _reference(guide, c, mean, var, radius, patch, K, 1)[0]
    if (nx, rows) != (1, 1):  # coverage, from the reference alone: a call that ignores `levels` fails
        assert (_bits(want) != _bits(one)).any(axis=-1).sum() >= min(89, nx * rows // 2)
    for s in range(levels):  # the inputs of every level first: a wrong downsample shows apart from a wrong combine
        got, (pc, pm, pv) = ctx.debug_denoise_multiscale(c, mean, var, levels, guide, radius, patch, K, probe_level=s)
        assert pc.shape[:2] == ref.level_size(nx, rows, s)[::-1]
        _same(pc, lv[s]["c"], (nx, rows, guide, levels, "c of level", s))
        if guide == "luminance":
            _same(pm, lv[s]["guides"][0][0], (nx, rows, levels, "y of level", s))
            _same(pv, lv[s]["guides"][0][1], (nx, rows, levels, "v of level", s))
        else:
            _same(pm, lv[s]["c"], (nx, rows, levels, "the guide means of level", s))
            _same(pv, np.stack([g[1] for g in lv[s]["guides"]], axis=-1), (nx, rows, levels, "the variances of level", s))
        _same(got, want, (nx, rows, radius, patch, guide, levels, "o_0, probing level", s))
    _same(ctx.debug_denoise_multiscale(c, mean, var, levels, guide, radius, patch, K), want, (nx, rows, radius, patch, guide, levels))


@pytest.mark.parametrize("guide", GUIDES)
def test_one_level_is_the_single_scale_kernel(ctx, guide):
    for nx, rows, radius, patch in [(37, 21, 5, 1), (35, 19, 3, 2), (1, 1, 5, 1)]:
        c, mean, var = _kernel_case(guide, nx, rows)
        single = ctx.debug_denoise(c, mean, var, radius, patch, K) if guide == "luminance" else ctx.debug_denoise_channels(c, var, radius, patch, K)
        _same(ctx.debug_denoise_multiscale(c, mean, var, 1, guide, radius, patch, K), single, (guide, nx, rows))


def test_the_debug_call_keeps_nothing_between_calls_and_refuses_what_the_header_says(rt, ctx):
    f = rt._ffi
    c, y, v = denoise_ref.kernel_case(37, 21)
    c3, _, var3 = _kernel_case("channels", 13, 9)
    first = ctx.debug_denoise_multiscale(c, y, v, 3, "luminance", 5, 1, K)
    between = ctx.debug_denoise_multiscale(c3, None, var3, 4, "channels", 5, 1, K)
    assert between.shape == c3.shape
    _same(ctx.debug_denoise_multiscale(c, y, v, 3, "luminance", 5, 1, K), first, "the first inputs again")
    for bad in (dict(levels=0), dict(levels=f.DENOISE_MAX_LEVELS + 1), dict(levels=2, guide=2), dict(levels=2, radius=0), dict(levels=2, probe_level=2)):
        _raises(rt, f.ERR_INVALID, ctx.debug_denoise_multiscale, c, y, v, **bad)


# ---- 2. the accumulation against the reference ----------------------------------------------------------------------------------------
def _accumulate(rt, r, case, adaptive):
    """Opens the accumulation of the case with channels tracked and adds 16 samples, or 8 and two adaptive adds of 8.  Returns the
    filter's inputs as the replay of the single-sample frames gives them: (c, y, v, var_rgb), all f32 in image order."""
    scene, prm = _setup(rt, r, case)
    x = _singles(r, scene, prm, case, 24 if adaptive else 16)
    rp = adaptive_ref.Replay(x)
    r.accum_begin(scene.camera, prm(8, spp_slice=6))
    r.accum_track_channels()
    if adaptive:
        floor = 0.01
        rel = adaptive_ref.relative_error(x, 8, floor)
        rel = rel[np.isfinite(rel) & (rel > 0)]
        tol = float(np.median(rel))
        r.accum_add(8), rp.uniform(8)
        for _ in range(2):
            r.accum_add_adaptive(8, tol, floor, 8), rp.adaptive(8, tol, floor, 8)
        counts, info = r.accum_counts()
        assert np.array_equal(counts, rp.cnt) and info.n_active < counts.size and len(np.unique(counts)) >= 2, ("the case went vacuous", info.n_active)
    else:
        r.accum_add(16), rp.uniform(16)
    c = rp.image()
    _same(r.accum_read()[0], c, (case, "the accumulated frame"))
    ybar, v = adaptive_ref.pixel_figures(rp.s1, rp.s2, rp.cnt)
    var = ch_ref.channel_variance(*ch_ref.accumulate_channels(x, rp.cnt), rp.cnt)
    return scene, prm, c, ybar.astype(F32), v.astype(F32), var.astype(F32)


@pytest.mark.parametrize("adaptive", [False, True], ids=["uniform", "adaptive"])
@pytest.mark.parametrize("case", list(FRAMES))
def test_accumulation_matches_the_reference_bit_for_bit(rt, ctx, case, adaptive):
    r = ctx
    _, _, c, y, v, var = _accumulate(rt, r, case, adaptive)
    k = rt._ffi.DENOISE_DEFAULT_STRENGTH
    single = {"luminance": r.accum_denoise(want_rgb8=True), "channels": r.accum_denoise_channels(want_rgb8=True)}
    for guide in GUIDES:
        for levels in (1, 2, 3, 4):
            want = (ref.luminance(c, y, v, 5, 1, k, levels) if guide == "luminance" else ref.channels(c, var, 5, 1, k, levels))[0]
            img, rgb8 = r.accum_denoise_multiscale(levels, guide, want_rgb8=True)
            _same(img, want, (case, guide, levels, "filtered f32"))
            _same(rgb8, denoise_ref.finalize_rgb8(want), (case, guide, levels, "filtered rgb8"))
            if levels == 1:
                _same(img, single[guide][0], (case, guide, "one level against the single-scale call"))
                _same(rgb8, single[guide][1], (case, guide, "one level against the single-scale call, rgb8"))
            else:
                assert (_bits(img) != _bits(single[guide][0])).any(axis=-1).mean() >= 0.5, (case, guide, levels, "coverage: the levels change little")
        img2, none = r.accum_denoise_multiscale(3, guide, 5, 1, None)
        assert none is None
        _same(img2, (ref.luminance(c, y, v, 5, 1, k, 3) if guide == "luminance" else ref.channels(c, var, 5, 1, k, 3))[0], (case, guide, "a second call"))
    r.accum_end()


# ---- 3. the accumulation is undisturbed -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guide", GUIDES)
def test_the_accumulation_is_undisturbed(rt, ctx, guide):
    r = ctx
    scene, prm = _setup(rt, r, "B")
    r.accum_begin(scene.camera, prm(7))
    r.accum_track_channels()
    r.accum_add(7)
    before = r.accum_read(want_rgb8=True, want_sem=True)
    sem_before = r.accum_channel_sem()
    filtered = r.accum_denoise_multiscale(4, guide, want_rgb8=True)[0]
    assert (filtered != before[0]).any()
    after = r.accum_read(want_rgb8=True, want_sem=True)
    for k, what in enumerate(("f32", "rgb8", "sem")):
        _same(after[k], before[k], (guide, what, "read after the filter"))
    assert bytes(after[3]) == bytes(before[3])
    _same(r.accum_channel_sem(), sem_before, "channel sem after the filter")
    r.accum_add(2)
    _same(r.accum_read()[0], r.render(scene.camera, prm(9))[0], (guide, "two more samples after the filter"))
    r.accum_end()


# ---- 4. state and arguments -----------------------------------------------------------------------------------------------------------
def test_state_and_arguments(rt, ctx):
    f = rt._ffi
    r = ctx
    scene, prm = _setup(rt, r, "A")
    r.accum_end()
    for guide in GUIDES:
        _raises(rt, f.ERR_STATE, r.accum_denoise_multiscale, 2, guide)  # no accumulation
    r.accum_begin(scene.camera, prm(1))
    r.accum_add(1)
    kept = r.accum_read()[0]
    _raises(rt, f.ERR_STATE, r.accum_denoise_multiscale)  # one sample: no variance yet
    _same(r.accum_read()[0], kept, "after the refusal at one sample")
    r.accum_add(6)
    _raises(rt, f.ERR_STATE, r.accum_denoise_multiscale, 2, "channels")  # channels are not tracked
    assert "does not track channels" in r._lib.rt_last_error(r._ctx).decode()
    kept = r.accum_read(want_rgb8=True)
    fp = C.POINTER(C.c_float)

    def raw(dn, ms, img=None):
        img = np.zeros_like(kept[0]) if img is None else img
        return r._lib.rt_accum_denoise_multiscale(r._ctx, C.byref(dn) if dn is not None else None, C.byref(ms) if ms is not None else None,
                                                  img.ctypes.data_as(fp), None), img

    good_dn, good_ms = f.RtDenoise(5, 1, 0.7, 0), f.RtMultiscale(2, f.DENOISE_GUIDE_LUMINANCE)
    bad_dn = [f.RtDenoise(0, 1, 0.7, 0), f.RtDenoise(f.DENOISE_MAX_RADIUS + 1, 1, 0.7, 0), f.RtDenoise(5, f.DENOISE_MAX_PATCH + 1, 0.7, 0),
              f.RtDenoise(5, 1, 0.0, 0), f.RtDenoise(5, 1, -1.0, 0), f.RtDenoise(5, 1, float("nan"), 0), f.RtDenoise(5, 1, float("inf"), 0),
              f.RtDenoise(5, 1, 0.7, 1)]
    bad_ms = [f.RtMultiscale(0, 0), f.RtMultiscale(f.DENOISE_MAX_LEVELS + 1, 0), f.RtMultiscale(2, 2), f.RtMultiscale(2, 0xFFFFFFFF),
              f.RtMultiscale(2, 0, (C.c_uint32 * 2)(1, 0)), f.RtMultiscale(2, 0, (C.c_uint32 * 2)(0, 1))]
    for dn, ms in [(d, good_ms) for d in bad_dn] + [(good_dn, m) for m in bad_ms] + [(None, m) for m in bad_ms]:
        rc, img = raw(dn, ms)
        assert rc == -f.ERR_INVALID and not img.any(), (rc, ms.levels, ms.guide, list(ms.reserved))
        again = r.accum_read(want_rgb8=True)
        _same(again[0], kept[0], "after a refused call")
        _same(again[1], kept[1], "after a refused call, rgb8")
    # the largest legal values pass, and NULL is the defaults
    assert raw(f.RtDenoise(f.DENOISE_MAX_RADIUS, f.DENOISE_MAX_PATCH, 0.7, 0), f.RtMultiscale(f.DENOISE_MAX_LEVELS, 0))[0] == 0
    rc, by_null = raw(None, None)
    assert rc == 0
    rc, by_hand = raw(f.RtDenoise(5, 1, f.DENOISE_DEFAULT_STRENGTH, 0), f.RtMultiscale(f.DENOISE_DEFAULT_LEVELS, f.DENOISE_GUIDE_LUMINANCE))
    assert rc == 0 and (by_null != kept[0]).any()
    _same(by_null, by_hand, "NULL against the explicit defaults")
    _same(r.accum_denoise_multiscale()[0], by_null, "the wrapper's defaults")
    assert (_bits(by_null) != _bits(r.accum_denoise()[0])).any(), "the default levels are more than one"
    assert r._lib.rt_accum_denoise_multiscale(r._ctx, None, None, None, None) == 0  # both outputs NULL: nothing to write, no error
    assert r._lib.rt_accum_denoise_multiscale(None, None, None, None, None) == -f.ERR_INVALID
    r.accum_add(2)
    _same(r.accum_read()[0], r.render(scene.camera, prm(9))[0], "the accumulation after all of it")
    # a sharded frame
    shard = prm(2, shard_count=2, shard_band=4, shard_id=1)
    r.accum_begin(scene.camera, shard)
    r.accum_add(2)
    kept = r.accum_read()[0]
    _raises(rt, f.ERR_UNSUPPORTED, r.accum_denoise_multiscale)
    _same(r.accum_read()[0], kept, "the shard after the refusal")
    r.accum_end()


# ---- 5. rendered frames: below the single-scale filter where it was measured lower ----------------------------------------------------
# RMSE against rt_render of the same scene at 4 096 spp with another seed, linear radiance, 16 spp, default parameters: the three frames
# of DESIGN.md 4.6.  MEASURED[frame][guide] = RMSE(filtered) / RMSE(16 spp) for 1, 2, 3 and 4 levels as measured on an MI355X (DESIGN.md
# 4.12); the frames are bit-reproducible.  Where more levels came out lower than one level, the test holds them below the single-scale
# figure of the same frame, computed here by the existing call, with the margin sqrt(measured ratio of the two * 1).  Where they came out
# no better — two levels on the 64 x 64 cornell_box with Scene.lights, either guide — nothing is asserted; 4.12 says so.
QUALITY_FRAMES = {
    "cornell_lights": dict(scene="cornell_box", nx=64, ny=64, depth=8, lights=True),
    "cornell_no_lights": dict(scene="cornell_box", nx=64, ny=64, depth=8, lights=False),
    "test_sphere": dict(scene="test_sphere", nx=64, ny=32, depth=50, lights=False),
}
MEASURED = {
    "cornell_lights": {"luminance": (0.4246, 0.4300, 0.4206, 0.4199), "channels": (0.4191, 0.4213, 0.4167, 0.4163)},
    "cornell_no_lights": {"luminance": (0.3528, 0.3514, 0.3412, 0.3435), "channels": (0.3518, 0.3414, 0.3363, 0.3383)},
    "test_sphere": {"luminance": (0.3808, 0.3725, 0.3616, 0.3606), "channels": (0.3828, 0.3733, 0.3625, 0.3615)},
}
_truth = {}


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("frame", list(QUALITY_FRAMES))
def test_more_levels_stay_below_the_single_scale_filter_where_measured_lower(rt, ctx, frame, guide):
    r = ctx
    q = QUALITY_FRAMES[frame]
    key = (q["scene"], q["nx"], q["ny"])
    if key not in _scenes:
        _scenes[key] = rt.Scene.build(q["scene"], q["nx"] / q["ny"])
    scene = _scenes[key]
    r.upload(scene)
    if q["lights"]:
        r.set_lights(scene.lights)
    if frame not in _truth:
        _truth[frame] = r.render(scene.camera, rt.make_params(q["nx"], q["ny"], 4096, max_depth=q["depth"], seed=SEED + 1))[0]
    truth = _truth[frame]
    r.accum_begin(scene.camera, rt.make_params(q["nx"], q["ny"], 16, max_depth=q["depth"], seed=SEED))
    r.accum_track_channels()
    r.accum_add(16)
    noisy = r.accum_read()[0]
    single = (r.accum_denoise() if guide == "luminance" else r.accum_denoise_channels())[0]
    filtered = {levels: r.accum_denoise_multiscale(levels, guide)[0] for levels in (2, 3, 4)}
    r.accum_end()
    r.set_lights(None)
    e_noisy, e_single = denoise_ref.rmse(noisy, truth), denoise_ref.rmse(single, truth)
    measured = MEASURED[frame][guide]
    print(f"{frame}, {guide}: RMSE {e_noisy:.5f}; 1 level {e_single / e_noisy:.4f}")
    asserted = 0
    for levels, img in filtered.items():
        e = denoise_ref.rmse(img, truth)
        print(f"  {levels} levels: ratio {e / e_noisy:.4f} (measured {measured[levels - 1]:.4f})")
        assert np.isfinite(img).all()
        if measured[levels - 1] < measured[0]:
            assert e <= e_single * np.sqrt(measured[levels - 1] / measured[0] * 1.0), (frame, guide, levels, e / e_noisy, e_single / e_noisy)
            asserted += 1
    assert asserted >= (2 if frame == "cornell_lights" else 3)
