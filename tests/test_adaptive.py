"""Adaptive sampling on the GPU (rt_accum_add_adaptive, rt_accum_read_counts, rt_render_adaptive).  tests/adaptive_ref.py replays every
accumulation over the single-sample frames the accumulation itself delivers through first_sample, and the GPU is held to it bit for
bit: sample counts, images, out_sem; the frame figures within the npix 2^-52 of a reordered sum.  The defining property — pixel p is
pixel p of rt_render with spp = n_p — is also held against rt_render directly.

Frames: 24 x 16 (tiles where the scene takes them; 384 pixels are no multiple of 256, so a chunk of primary rays straddles two samples),
20 x 10 (row-major, fewer pixels than a chunk), a shard of 8 rows, 1 x 1.  Steps of 6 samples, at most 24.

The tolerance of a case is chosen from the reference alone: a quantile (the median, unless the case names another), over the pixels with any
variance, of the relative standard error sqrt(V) / max(Ybar, floor) after 12 samples — the middle decision — so that some pixels stop
early, some at the middle and some never; the coverage is asserted on the reference's counts, never on the GPU's."""
import numpy as np
import pytest

import adaptive_ref
import denoise_ref
import helpers
import noise_ref

pytestmark = pytest.mark.gpu

SEED, FLOOR, MIN, STEP, MAX = 4321, 0.01, 6, 6, 24
BRUTE = 1  # RT_FLAG_BRUTE_FORCE
CASES = {
    "grid": dict(scene="sphere_scene", nx=24, ny=16, kw=dict(max_depth=50)),                  # sphere grid, two chains, 8 x 8 tiles
    "tree": dict(scene="cornell_box", nx=24, ny=16, kw=dict(max_depth=8)),                    # tree, one chain, wrappers, rows
    "medium": dict(scene="final_scene", nx=20, ny=10, kw=dict(max_depth=50), q=0.1),   # (86 % of this view is black: a low quantile)
    "lens": dict(scene="test_sphere", nx=20, ny=10, kw=dict(max_depth=50), lens=(0.05, 3.0)),
    "lights": dict(scene="cornell_box", nx=24, ny=16, kw=dict(max_depth=8), lights=True),
    "quads": dict(scene="quads_scene", nx=24, ny=16, kw=dict(max_depth=8), quads=True),
    "motion": dict(scene="moving_sphere_scene", nx=24, ny=16, kw=dict(max_depth=8), motion=True),
    "brute": dict(scene="test_sphere", nx=24, ny=16, kw=dict(max_depth=50, flags=BRUTE)),
    "shard": dict(scene="test_sphere", nx=24, ny=16, kw=dict(max_depth=50, shard_count=2, shard_band=4, shard_id=1)),
    "one": dict(scene="test_sphere", nx=1, ny=1, kw=dict(max_depth=50)),
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


_scenes, _single = {}, {}


def _setup(rt, r, case):
    c = CASES[case]
    key = (c["scene"], c["nx"], c["ny"])
    if key not in _scenes:
        _scenes[key] = rt.Scene.build(c["scene"], c["nx"] / c["ny"])
    scene = _scenes[key]
    r.upload(scene)
    r.set_lens(c.get("lens"))
    if c.get("lights"):
        r.set_lights(scene.lights)
    if c.get("quads"):
        assert scene.quads.n
        r.set_quads(scene.quads)
    if c.get("motion"):
        assert scene.motion.n_moving
        r.set_motion(scene.motion)
    return scene, lambda spp, **kw: rt.make_params(c["nx"], c["ny"], spp, seed=SEED, **{"spp_slice": 4, **c["kw"], **kw})


def _singles(r, scene, prm, case, n=MAX):
    """x[s], s < n: the single-sample frames of the case (computed once, never changed)."""
    have = _single.setdefault(case, [])
    for s in range(len(have), n):
        r.accum_begin(scene.camera, prm(1), first_sample=s)
        r.accum_add(1)
        img = r.accum_read()[0]
        img.setflags(write=False)
        have.append(img)
    r.accum_end()
    return have[:n]


def _tolerance(x, case=None):
    rel = adaptive_ref.relative_error(x, 12, FLOOR)
    rel = rel[np.isfinite(rel) & (rel > 0)]
    return float(np.quantile(rel, CASES.get(case, {}).get("q", 0.5))) if rel.size else 0.05


def _check(r, rp, what, stats=None):
    """The open accumulation against the replay: counts, images, sem bit for bit, the figures within a reordered sum, the integer sums."""
    img, rgb8, sem, noise = r.accum_read(want_rgb8=True, want_sem=True)
    counts, info = r.accum_counts()
    assert np.array_equal(counts, rp.cnt), (what, "counts", int((counts != rp.cnt).sum()))
    _same(img, rp.image(), (what, "f32"))
    _same(rgb8, denoise_ref.finalize_rgb8(rp.image()), (what, "rgb8"))
    _same(sem, rp.sem(), (what, "sem"))
    assert (info.n_active, info.n_samples, info.spp_min, info.spp_max) == rp.info(), (what, "info")
    assert noise.spp_done == rp.info()[3] and noise.reserved == 0
    mean, rms, nz = rp.frame_figures()
    print(f"{what}: counts {np.unique(counts, return_counts=True)}, mean {noise.mean_luminance!r} / {mean!r}, rms_sem {noise.rms_sem!r} / {rms!r}, "
          f"noise {noise.noise!r} / {nz!r}")
    tol = counts.size * 2.0 ** -52
    for got, want in ((noise.mean_luminance, mean), (noise.rms_sem, rms), (noise.noise, nz)):
        assert (np.isnan(got) and np.isnan(want)) or got == want or abs(got - want) <= tol * abs(want), (what, got, want)
    if stats is not None:
        assert stats.n_paths == rp.traced[-1] == stats.rays_per_depth[0], (what, stats.n_paths, rp.traced[-1])
    return img, sem, counts, noise


def _run(r, scene, prm, x, steps, tol, floor=FLOOR, mn=MIN, what=""):
    """steps: ("u", n) a uniform add, ("a", n) an adaptive one.  Both sides, compared after every step.  Leaves the accumulation open."""
    rp = adaptive_ref.Replay(x)
    r.accum_begin(scene.camera, prm(STEP))
    for k, (kind, n) in enumerate(steps):
        if kind == "u":
            st = r.accum_add(n)
            rp.uniform(n)
        else:
            st = r.accum_add_adaptive(n, tol, floor, mn)
            rp.adaptive(n, tol, floor, mn)
        _check(r, rp, (what, k, kind, n), st)
    return rp


# ---- 1. the defining property, per scene class -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_pixel_p_is_pixel_p_of_a_render_with_its_own_count(rt, ctx, case):
    r = ctx
    scene, prm = _setup(rt, r, case)
    x = _singles(r, scene, prm, case)
    tol = _tolerance(x, case)
    rp = _run(r, scene, prm, x, [("a", STEP)] * (MAX // STEP), tol, what=case)
    cnt = rp.cnt
    if cnt.size >= 100:  # coverage, from the reference alone
        early, full, middle = (cnt < MAX).mean(), (cnt == MAX).mean(), ((cnt > MIN) & (cnt < MAX)).sum()
        assert early >= 0.10 and full >= 0.10 and middle >= 1, (case, tol, early, full, middle)
    img, _, sem, _ = r.accum_read(want_sem=True)
    for n in np.unique(cnt):  # rt_render itself, while the accumulation stays open
        m = cnt == n
        want = r.render(scene.camera, prm(int(n)))[0]
        assert np.array_equal(_bits(img)[m], _bits(want)[m]), (case, "rt_render with spp", int(n))
        assert np.array_equal(_bits(sem)[m], _bits(noise_ref.sem(*noise_ref.accumulate(x[:int(n)])[1:]))[m]), (case, "sem at", int(n))
    again = r.accum_read(want_sem=True)
    _same(again[0], img, (case, "after the renders in between"))
    r.accum_end()


# ---- 2. edges of the decision -------------------------------------------------------------------------------------------------------------
def test_tolerance_zero_stops_only_pixels_without_variance(rt, ctx):
    r = ctx
    scene, prm = _setup(rt, r, "tree")
    x = _singles(r, scene, prm, "tree")
    flat = noise_ref.sem(*noise_ref.accumulate(x[:MIN])[1:]) == 0
    assert flat.any() and not flat.all(), "coverage: cornell_box has pixels without variance after 6 samples, and others"
    rp = _run(r, scene, prm, x, [("a", STEP)] * (MAX // STEP), 0.0, what="tolerance 0")
    assert ((rp.cnt < MAX) <= flat).all() and (rp.cnt == MIN)[flat].all()
    img = r.accum_read()[0]
    want = r.render(scene.camera, prm(MAX))[0]
    assert np.array_equal(_bits(img)[rp.cnt == MAX], _bits(want)[rp.cnt == MAX])
    r.accum_end()


def test_a_huge_tolerance_stops_everything_and_the_next_add_traces_nothing(rt, ctx):
    r = ctx
    scene, prm = _setup(rt, r, "grid")
    x = _singles(r, scene, prm, "grid")
    rp = _run(r, scene, prm, x, [("a", STEP), ("a", STEP)], 1e30, what="huge tolerance")
    assert (rp.cnt == MIN).all() and rp.traced == [rp.cnt.size * STEP, 0]
    before = r.accum_read(want_rgb8=True, want_sem=True)
    st = r.accum_add_adaptive(STEP, 1e30, FLOOR, MIN)
    assert st.n_paths == 0 and st.n_rays == 0 and r.accum_counts()[1].n_active == 0
    after = r.accum_read(want_rgb8=True, want_sem=True)
    for k in range(3):
        _same(after[k], before[k], ("an add that traces nothing", k))
    assert bytes(after[3]) == bytes(before[3])
    r.accum_end()


@pytest.mark.parametrize("case", ["grid", "tree"])
def test_one_nan_pixel_stays_active_alone_and_does_not_spread(rt, ctx, case):
    r = ctx
    scene, prm = _setup(rt, r, case)
    x = _singles(r, scene, prm, case)
    rp = adaptive_ref.Replay(x)
    r.accum_begin(scene.camera, prm(STEP))
    r.accum_add(MIN), rp.uniform(MIN)
    pixel = 5 * CASES[case]["nx"] + 7
    r.debug_accum_set_moments(pixel, float("nan"), float("nan")), rp.set_moments(pixel, np.nan, np.nan)
    for k in range(2):  # exactly one active pixel: one chunk of the generator holds all the rays there are
        st = r.accum_add_adaptive(STEP, 1e30, FLOOR, MIN)
        assert rp.adaptive(STEP, 1e30, FLOOR, MIN) == 1
        assert st.n_paths == STEP
        img, sem, counts, noise = _check(r, rp, (case, "one active pixel", k), st)
    assert counts.reshape(-1)[pixel] == MIN + 2 * STEP and (np.delete(counts.reshape(-1), pixel) == MIN).all()
    assert np.isnan(sem.reshape(-1)[pixel]) and np.isfinite(np.delete(sem.reshape(-1), pixel)).all() and np.isnan(noise.noise)
    want = r.render(scene.camera, prm(MIN + 2 * STEP))[0]  # its f32 sum was not touched: still the pixel of a render
    assert np.array_equal(_bits(img).reshape(-1, 3)[pixel], _bits(want).reshape(-1, 3)[pixel])
    r.accum_end()


@pytest.mark.parametrize("name,steps,mn", [
    ("min_samples no multiple of the step", [("a", 6)] * 4, 8),
    ("a uniform warm-up", [("u", 5), ("a", 6), ("a", 6), ("a", 7)], 6),
    ("uneven adds", [("u", 2), ("u", 1), ("a", 1), ("a", 9), ("a", 3), ("a", 8)], 4),
])
def test_schedules(rt, ctx, name, steps, mn):
    r = ctx
    for case in ("grid", "tree"):
        scene, prm = _setup(rt, r, case)
        x = _singles(r, scene, prm, case)
        rp = _run(r, scene, prm, x, steps, _tolerance(x), mn=mn, what=(case, name))
        assert (rp.cnt < MAX).any() and (rp.cnt == MAX).any(), (case, name, "coverage")
        stops = set(np.unique(rp.stopped_at).tolist()) - {-1}
        decisions, n = set(), 0
        for kind, k in steps:
            if kind == "a" and n >= mn:
                decisions.add(n)
            n += k
        assert stops and stops <= decisions, (case, name, stops, decisions)
        r.accum_end()


# ---- 3. order independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["grid", "tree", "lens"])
def test_the_place_in_the_queue_changes_no_bit(rt, case):
    r = rt.Renderer(0)  # (a context of its own: the options of the shared one stay)
    try:
        scene, prm = _setup(rt, r, case)
        x = _singles(r, scene, prm, case)
        tol = _tolerance(x)

        def render(options, **kw):
            for opt in rt._ffi.OPT_NAMES.values():
                r.set_option(opt, 0)
            for opt, value in options.items():
                r.set_option(opt, value)
            return r.render_adaptive(scene.camera, prm(MAX, **kw), tol, STEP, FLOOR, MIN, want_rgb8=True, want_sem=True)

        base = render({})
        assert (base[3] < MAX).any() and (base[3] == MAX).any()
        settings = [({}, {}), ({"queue_shards": 7}, {}), ({"queue_shards": 9}, {}), ({"queue_shards": 9, "isect_workgroups": 1}, {}),
                    ({"chains": 1}, {}), ({"chains": 2}, {}), ({"isect_workgroups": 3}, {}), ({"pixel_order": 1}, {}), ({"pixel_order": 2}, {}),
                    ({}, {"spp_slice": 1}), ({}, {"spp_slice": 0}), ({"materialise_primaries": 1}, {}), ({"primary_lists": 1}, {})]
        for options, kw in settings:
            got = render(options, **kw)
            for k, name in enumerate(("f32", "rgb8", "sem", "counts")):
                _same(got[k], base[k], (case, options, kw, name))
            assert bytes(got[4]) == bytes(base[4]) and bytes(got[5]) == bytes(base[5]), (case, options, kw, "figures and info")
            assert got[6].n_paths == base[6].n_paths and list(got[6].rays_per_depth) == list(base[6].rays_per_depth), (case, options, kw)
    finally:
        r.close()


# ---- 4. reading and denoising -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["grid", "tree"])
def test_reading_twice_and_denoising(rt, ctx, case):
    r = ctx
    scene, prm = _setup(rt, r, case)
    x = _singles(r, scene, prm, case)
    rp = _run(r, scene, prm, x, [("a", STEP)] * 3, _tolerance(x), what=(case, "denoise"))
    assert len(np.unique(rp.cnt)) >= 2
    one, two = r.accum_read(want_rgb8=True, want_sem=True), r.accum_read(want_rgb8=True, want_sem=True)
    for k in range(3):
        _same(one[k], two[k], (case, "second read", k))
    assert bytes(one[3]) == bytes(two[3]) and bytes(r.accum_counts()[1]) == bytes(r.accum_counts()[1])
    ybar, v = adaptive_ref.pixel_figures(rp.s1, rp.s2, rp.cnt)
    want, _ = denoise_ref.denoise(rp.image(), ybar.astype(np.float32), v.astype(np.float32), 5, 1, rt._ffi.DENOISE_DEFAULT_STRENGTH)
    assert (want != rp.image()).any()
    img, rgb8 = r.accum_denoise(want_rgb8=True)
    _same(img, want, (case, "filtered f32"))
    _same(rgb8, denoise_ref.finalize_rgb8(want), (case, "filtered rgb8"))
    three = r.accum_read(want_rgb8=True, want_sem=True)
    for k in range(3):
        _same(three[k], one[k], (case, "read after the filter", k))
    st = r.accum_add_adaptive(STEP, _tolerance(x), FLOOR, MIN)  # and the adds go on
    rp.adaptive(STEP, _tolerance(x), FLOOR, MIN)
    _check(r, rp, (case, "an add after the filter"), st)
    r.accum_end()


# ---- 5. rt_render_adaptive ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["grid", "tree", "shard"])
def test_render_adaptive_equals_the_manual_loop(rt, ctx, case):
    r = ctx
    scene, prm = _setup(rt, r, case)
    x = _singles(r, scene, prm, case)
    tol = _tolerance(x)
    # to the maximum: some pixel is still active after the last decision
    rp = adaptive_ref.Replay(x)
    active = [rp.adaptive(n, tol, FLOOR, MIN) for n in (STEP, STEP, STEP, STEP)]
    assert active[-1] > 0
    img, rgb8, sem, counts, noise, info, st = r.render_adaptive(scene.camera, prm(MAX), tol, STEP, FLOOR, MIN, want_rgb8=True, want_sem=True)
    _raises(rt, rt._ffi.ERR_STATE, r.accum_read)  # it ended its accumulation
    assert np.array_equal(counts, rp.cnt) and noise.spp_done == MAX and (info.n_active, info.n_samples, info.spp_min, info.spp_max) == rp.info()
    _same(img, rp.image(), (case, "f32")), _same(sem, rp.sem(), (case, "sem")), _same(rgb8, denoise_ref.finalize_rgb8(rp.image()), (case, "rgb8"))
    assert st.n_paths == sum(rp.traced) == info.n_samples
    # a maximum that is no multiple of the step: the last add takes what is left
    rp = adaptive_ref.Replay(x)
    for n in (5, 5, 5, 5, 2):
        rp.adaptive(n, tol, FLOOR, MIN)
    got = r.render_adaptive(scene.camera, prm(22), tol, 5, FLOOR, MIN, want_sem=True)
    assert np.array_equal(got[3], rp.cnt) and got[4].spp_done == 22
    _same(got[0], rp.image(), (case, "22 samples in steps of 5"))
    # a tolerance under which every pixel stops: the loop ends with the add that finds nobody active, at the count the reference predicts
    rp = adaptive_ref.Replay(x)
    active = [rp.adaptive(STEP, 1e30, FLOOR, 8) for _ in range(3)]
    assert active == [rp.cnt.size, rp.cnt.size, 0]
    got = r.render_adaptive(scene.camera, prm(MAX), 1e30, STEP, FLOOR, 8)
    assert got[4].spp_done == 12 == rp.info()[3] and got[5].n_active == 0 and np.array_equal(got[3], rp.cnt)
    _same(got[0], rp.image(), (case, "everything stops at 12"))
    _same(got[0], r.render(scene.camera, prm(12))[0], (case, "everything stops at 12: rt_render"))
    assert got[6].n_paths == rp.cnt.size * 12


def test_render_adaptive_sums_the_statistics_of_its_adds(rt, ctx):
    """22 samples at the most in steps of 5: the adds are 5, 5, 5, 5 and 2, the last one short, each on the pixels still active."""
    r = ctx
    scene, prm = _setup(rt, r, "tree")
    tol = _tolerance(_singles(r, scene, prm, "tree"))
    r.accum_begin(scene.camera, prm(5))
    adds = [r.accum_add_adaptive(n, tol, FLOOR, MIN) for n in (5, 5, 5, 5, 2)]
    counts = r.accum_counts()[0]
    r.accum_end()
    assert 0 < adds[-1].n_paths < adds[0].n_paths == counts.size * 5  # (some pixels stopped, some run to the maximum)
    got = r.render_adaptive(scene.camera, prm(22), tol, 5, FLOOR, MIN)
    total = got[6]
    assert np.array_equal(got[3], counts) and total.n_paths == int(counts.sum())
    helpers.stats_are_the_sum(total, adds, "render_adaptive")


# ---- 6. state machine and errors ------------------------------------------------------------------------------------------------------------
def test_state_and_arguments(rt, ctx):
    f = rt._ffi
    r = ctx
    bare = rt.Renderer(0)
    try:
        _raises(rt, f.ERR_STATE, bare.accum_add_adaptive, 1, 0.1)
        # a NULL RtAdaptive: refused by the state first, under the adaptive add's own name (both adds share their host path)
        assert bare._lib.rt_accum_add_adaptive(bare._ctx, 1, None, None) == -f.ERR_STATE
        assert bare._lib.rt_last_error(bare._ctx).decode().startswith("rt_accum_add_adaptive: no accumulation begun")
        _raises(rt, f.ERR_STATE, bare.accum_counts)
        _raises(rt, f.ERR_STATE, bare.render_adaptive, _scenes_any(rt).camera, rt.make_params(24, 16, 4), 0.1, 2)  # no scene
    finally:
        bare.close()
    scene, prm = _setup(rt, r, "grid")
    x = _singles(r, scene, prm, "grid")
    tol = _tolerance(x)
    _raises(rt, f.ERR_STATE, r.accum_add_adaptive, 1, 0.1)
    _raises(rt, f.ERR_STATE, r.accum_counts)
    # before the first adaptive add: the counts of a uniform accumulation
    r.accum_begin(scene.camera, prm(STEP))
    assert r._lib.rt_accum_add_adaptive(r._ctx, 1, None, None) == -f.ERR_INVALID  # (not taken for a uniform add: nothing was added)
    assert r._lib.rt_last_error(r._ctx).decode() == "rt_accum_add_adaptive: the RtAdaptive is NULL"
    counts, info = r.accum_counts()
    assert not counts.any() and (info.n_active, info.n_samples, info.spp_min, info.spp_max) == (counts.size, 0, 0, 0)
    r.accum_add(3)
    counts, info = r.accum_counts()
    assert (counts == 3).all() and (info.n_active, info.n_samples, info.spp_min, info.spp_max) == (counts.size, 3 * counts.size, 3, 3)
    # each invalid parameter is refused and changes nothing
    before = r.accum_read(want_sem=True)
    bad = [dict(n=0), dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(tolerance=float("inf")), dict(luminance_floor=0.0),
           dict(luminance_floor=float("nan")), dict(min_samples=1), dict(min_samples=0)]
    for b in bad:
        _raises(rt, f.ERR_INVALID, r.accum_add_adaptive, **{**dict(n=STEP, tolerance=tol, luminance_floor=FLOOR, min_samples=MIN), **b})
    after = r.accum_read(want_sem=True)
    _same(after[0], before[0], "after the refused adds"), _same(after[2], before[2], "after the refused adds, sem")
    assert bytes(after[3]) == bytes(before[3])
    r.accum_add(3)  # still uniform: the refused adds did not make it adaptive
    # a uniform add after an adaptive one
    r.accum_add_adaptive(STEP, tol, FLOOR, MIN)
    kept = r.accum_read(want_sem=True), r.accum_counts()[0]
    _raises(rt, f.ERR_STATE, r.accum_add, 1)
    _same(r.accum_read()[0], kept[0][0], "after the refused uniform add")
    assert np.array_equal(r.accum_counts()[0], kept[1])
    # rt_render in between disturbs nothing, and is not disturbed
    two = r.render(scene.camera, prm(2))[0]
    _same(r.accum_read()[0], kept[0][0], "around a render")
    r.accum_add_adaptive(STEP, tol, FLOOR, MIN)
    rp = adaptive_ref.Replay(x)
    rp.uniform(6), rp.adaptive(STEP, tol, FLOOR, MIN), rp.adaptive(STEP, tol, FLOOR, MIN)
    _check(r, rp, "around a render")
    _same(r.render(scene.camera, prm(2))[0], two, "the render in between")
    # the bound of spp holds for an adaptive add
    r.accum_begin(scene.camera, prm(1), first_sample=2 ** 32 - 2)
    r.accum_add_adaptive(1, tol, FLOOR, MIN)
    _raises(rt, f.ERR_INVALID, r.accum_add_adaptive, 1, tol, FLOOR, MIN)
    assert r.accum_counts()[1].spp_max == 1
    # rt_render_adaptive: its arguments, and an open accumulation
    _raises(rt, f.ERR_STATE, r.render_adaptive, scene.camera, prm(8), tol, 4)
    r.accum_end()
    for kw, spp, step in ((dict(tolerance=tol), 8, 0), (dict(tolerance=-1.0), 8, 4), (dict(tolerance=tol, min_samples=1), 8, 4),
                          (dict(tolerance=tol, luminance_floor=-1.0), 8, 4), (dict(tolerance=tol), 1, 4)):
        _raises(rt, f.ERR_INVALID, r.render_adaptive, scene.camera, prm(spp), kw.pop("tolerance"), step, **kw)
        _raises(rt, f.ERR_STATE, r.accum_read)  # (none was left open)
    # what ends an accumulation ends an adaptive one; a new one starts uniform
    enders = [("upload", lambda: r.upload(scene)), ("set_lens", lambda: r.set_lens(None)), ("set_motion", lambda: r.set_motion(None)),
              ("set_quads", lambda: r.set_quads(None)), ("set_lights", lambda: r.set_lights(None)),
              ("set_option", lambda: r.set_option("chains", 0)), ("accum_end", r.accum_end)]
    for name, end in enders:
        r.accum_begin(scene.camera, prm(STEP))
        r.accum_add_adaptive(STEP, tol, FLOOR, MIN)
        end()
        _raises(rt, f.ERR_STATE, r.accum_add_adaptive, 1, tol, FLOOR, MIN)
        _raises(rt, f.ERR_STATE, r.accum_counts)
        _raises(rt, f.ERR_STATE, r.accum_read)
        r.accum_begin(scene.camera, prm(2))
        r.accum_add(2)  # uniform again
        _same(r.accum_read()[0], two, (name, "a new accumulation"))
        r.accum_end()


def _scenes_any(rt):
    return next(iter(_scenes.values())) if _scenes else rt.Scene.build("test_sphere", 1.5)


@pytest.mark.parametrize("case", ["grid", "tree", "lights", "lens"])
def test_an_adaptive_add_launches_what_a_materialised_frame_launches(rt, case):
    tables = rt.variant_tables()
    assert [len(tables[k]) for k in ("shade", "intersect", "debug_bounce", "untabled")] == [66, 66, 15, 7]
    r = rt.Renderer(0)
    try:
        scene, prm = _setup(rt, r, case)
        r.set_option("materialise_primaries", 1)
        r.launched_variants(reset=True)
        r.render(scene.camera, prm(STEP))
        frame = r.launched_variants(reset=True)
        assert frame["shade"] and not frame["debug_bounce"]
        r.set_option("materialise_primaries", 0)
        r.accum_begin(scene.camera, prm(STEP))
        r.launched_variants(reset=True)
        r.accum_add_adaptive(STEP, 0.05, FLOOR, MIN)
        r.accum_add_adaptive(STEP, 0.05, FLOOR, MIN)
        r.accum_read(want_rgb8=True, want_sem=True), r.accum_counts()
        got = r.launched_variants(reset=True)
        for fam in ("shade", "intersect", "debug_bounce", "untabled"):
            assert set(got[fam]) <= set(frame[fam]), (case, fam, set(got[fam]) - set(frame[fam]))
        assert got["shade"] == frame["shade"]
        r.accum_end()
    finally:
        r.close()
