"""Progressive accumulation, the per-pixel error estimate and the noise target (rt_accum_*, rt_render_to_noise) on the GPU.
Images are held to rt_render of the same context, bit for bit; moments to tests/noise_ref.py over single-sample frames, which the
accumulation itself delivers through first_sample.  The frames are the smallest that run both branches of the pixel order (case A:
40 x 20, sixteen rows in 8 x 8 tiles and four row-major), a general scene on one chain (B), a shard (C) and the sets (D)."""
import numpy as np
import pytest

import helpers
import noise_ref

pytestmark = pytest.mark.gpu

CASES = {
    "A": dict(scene="test_sphere", nx=40, ny=20, kw=dict(max_depth=50)),
    "B": dict(scene="cornell_box", nx=24, ny=16, kw=dict(max_depth=8)),
    "C": dict(scene="test_sphere", nx=40, ny=20, kw=dict(max_depth=50, shard_count=2, shard_band=4, shard_id=1)),
    "D_lights": dict(scene="cornell_box", nx=24, ny=16, kw=dict(max_depth=8), lights=True),
    "D_lens": dict(scene="test_sphere", nx=40, ny=20, kw=dict(max_depth=50), lens=(0.05, 3.0)),
}
SEED = 1234


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()), "values differ")


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


_scenes, _single = {}, {}


def _setup(rt, r, case):
    """Uploads the case's scene with its sets; returns (scene, params(spp))."""
    c = CASES[case]
    if c["scene"] not in _scenes:
        _scenes[c["scene"]] = rt.Scene.build(c["scene"], c["nx"] / c["ny"])
    scene = _scenes[c["scene"]]
    r.upload(scene)
    r.set_lens(c.get("lens"))
    if c.get("lights"):
        r.set_lights(scene.lights)
    return scene, lambda spp, **kw: rt.make_params(c["nx"], c["ny"], spp, seed=SEED, **{"spp_slice": 3, **c["kw"], **kw})


def _singles(r, scene, prm, case, n):
    """x[s], s < n: the single-sample frames of the case, each an accumulation of one sample that begins at s (computed once)."""
    have = _single.setdefault(case, [])
    for s in range(len(have), n):
        r.accum_begin(scene.camera, prm(1), first_sample=s)
        r.accum_add(1)
        img, _, sem, noise = r.accum_read(want_sem=True)
        assert noise.spp_done == 1 and noise.noise == np.inf and not sem.any()  # n = 1: no variance estimate, V = 0
        have.append(img)
    r.accum_end()
    return have[:n]


@pytest.mark.parametrize("case", list(CASES))
def test_continuation_equals_one_render(rt, ctx, case):
    r = ctx
    scene, prm = _setup(rt, r, case)
    want = {n: r.render(scene.camera, prm(n), want_rgb8=True) for n in (1, 3, 7)}
    r.accum_begin(scene.camera, prm(2))
    done = 0
    for n in (1, 2, 4):  # spp_slice = 3: the add of 4 is cut in two slices
        st = r.accum_add(n)
        done += n
        img, rgb8, _, noise = r.accum_read(want_rgb8=True)
        assert noise.spp_done == done and st.n_paths == img.shape[0] * img.shape[1] * n
        _same(img, want[done][0], (case, "f32 after", done))
        _same(rgb8, want[done][1], (case, "rgb8 after", done))
    assert st.n_slices == 2
    r.accum_begin(scene.camera, prm(7))  # (begin on an open accumulation starts over)
    st = r.accum_add(7)
    img, rgb8, _, _ = r.accum_read(want_rgb8=True)
    _same(img, want[7][0], (case, "one add"))
    _same(rgb8, want[7][1], (case, "one add, rgb8"))
    assert st.n_rays == want[7][2].n_rays and list(st.rays_per_depth) == list(want[7][2].rays_per_depth) and st.n_slices == 3
    r.accum_end()


@pytest.mark.parametrize("case", list(CASES))
def test_single_samples_and_moments(rt, ctx, case):
    r = ctx
    scene, prm = _setup(rt, r, case)
    x = _singles(r, scene, prm, case, 7)
    _same(x[0], r.render(scene.camera, prm(1))[0], (case, "x[0]"))
    total, s1, s2, n = noise_ref.accumulate(x)
    _same((total / np.float32(7)).astype(np.float32), r.render(scene.camera, prm(7))[0], (case, "sequential f32 sum of the single samples"))
    # a window that begins at sample 3
    r.accum_begin(scene.camera, prm(4), first_sample=3)
    r.accum_add(1), r.accum_add(3)
    win, _, _, noise = r.accum_read()
    assert noise.spp_done == 4
    _same(win, (noise_ref.accumulate(x[3:])[0] / np.float32(4)).astype(np.float32), (case, "window 3..6"))
    # moments of the 7-sample accumulation, added in portions
    r.accum_begin(scene.camera, prm(7))
    for k in (2, 4, 1):
        r.accum_add(k)
    _, _, sem, noise = r.accum_read(want_sem=True)
    want_sem = noise_ref.sem(s1, s2, 7)
    npix = want_sem.size
    assert (want_sem > 0).sum() >= 0.1 * npix, "coverage: the reference has too few noisy pixels"
    if case == "B":
        assert (want_sem == 0).any(), "coverage: the reference has no pixel without variance"
    _same(sem, want_sem, (case, "sem"))
    mean, rms, nz = noise_ref.frame_figures(s1, s2, 7)
    tol = npix * 2.0 ** -52
    print(f"{case}: mean {noise.mean_luminance!r} / {mean!r}, rms_sem {noise.rms_sem!r} / {rms!r}, noise {noise.noise!r} / {nz!r}")
    assert noise.spp_done == 7 and noise.reserved == 0
    assert abs(noise.mean_luminance - mean) <= tol * mean and abs(noise.rms_sem - rms) <= tol * rms and abs(noise.noise - nz) <= tol * nz
    _, _, sem2, noise2 = r.accum_read(want_sem=True)  # reading twice: the same bits
    _same(sem2, sem, (case, "second read"))
    assert bytes(noise2) == bytes(noise)
    r.accum_end()


def test_noise_falls_and_the_stopping_rule(rt, ctx):
    r = ctx
    scene, prm = _setup(rt, r, "B")
    x = _singles(r, scene, prm, "B", 64)
    ref = {n: noise_ref.noise_of(x[:n])[2] for n in (4, 8, 12, 16, 64)}
    print("noise_ref:", ref)
    # the reference first: 1 / sqrt(n), loosely (a guard against a wrong n, not a measurement)
    assert ref[4] > ref[16] > ref[64] and ref[16] / 1.5 <= 2.0 * ref[64] <= ref[16] * 1.5, ref
    r.accum_begin(scene.camera, prm(16))
    got = {}
    for n, add in ((4, 4), (16, 12), (64, 48)):
        r.accum_add(add)
        got[n] = r.accum_read()[3].noise
    r.accum_end()
    print("accumulated:", got)
    assert got[4] > got[16] > got[64] and got[16] / 1.5 <= 2.0 * got[64] <= got[16] * 1.5, got
    for n in got:
        assert abs(got[n] - ref[n]) <= 384 * 2.0 ** -52 * ref[n]
    # stopping: a target between the noise after 8 and after 12 samples ends the third step of 4
    assert ref[12] < ref[8], ref
    target = float(np.sqrt(ref[8] * ref[12]))
    img, rgb8, sem, noise, st = r.render_to_noise(scene.camera, prm(32), target, 4, want_rgb8=True, want_sem=True)
    want = r.render(scene.camera, prm(12), want_rgb8=True)
    assert noise.spp_done == 12 and noise.noise <= target
    _same(img, want[0], "render_to_noise, 12 samples")
    _same(rgb8, want[1], "render_to_noise, 12 samples, rgb8")
    _same(sem, noise_ref.sem(*noise_ref.accumulate(x[:12])[1:]), "render_to_noise, sem")
    assert st.n_rays == want[2].n_rays and st.n_paths == want[2].n_paths and list(st.rays_per_depth) == list(want[2].rays_per_depth)
    img, _, _, noise, st = r.render_to_noise(scene.camera, prm(32), 0.0, 4)
    assert noise.spp_done == 32
    _same(img, r.render(scene.camera, prm(32))[0], "render_to_noise, target 0")
    img, _, _, noise, _ = r.render_to_noise(scene.camera, prm(32), float("inf"), 4)
    assert noise.spp_done == 4
    _same(img, r.render(scene.camera, prm(4))[0], "render_to_noise, target inf")
    # a maximum that is no multiple of the step: the last add takes what is left
    assert r.render_to_noise(scene.camera, prm(10), 0.0, 4)[3].spp_done == 10


def test_render_to_noise_sums_the_statistics_of_its_adds(rt, ctx):
    """10 samples at the most in steps of 4, target 0: the adds are 4, 4 and 2, the last one short."""
    r = ctx
    scene, prm = _setup(rt, r, "B")
    r.accum_begin(scene.camera, prm(4))
    adds = [r.accum_add(n) for n in (4, 4, 2)]
    by_hand = r.accum_read()[0]
    r.accum_end()
    img, _, _, noise, total = r.render_to_noise(scene.camera, prm(10), 0.0, 4)
    assert noise.spp_done == 10 and total.n_paths == 24 * 16 * 10 and total.n_slices == sum(s.n_slices for s in adds) >= 3
    _same(img, by_hand, "render_to_noise against the same adds by hand")
    helpers.stats_are_the_sum(total, adds, "render_to_noise")


@pytest.mark.parametrize("case", ["A", "B"])
def test_render_in_between(rt, ctx, case):
    r = ctx
    scene, prm = _setup(rt, r, case)
    two, seven = r.render(scene.camera, prm(2))[0], r.render(scene.camera, prm(7))[0]
    r.accum_begin(scene.camera, prm(4))
    r.accum_add(3)
    _same(r.render(scene.camera, prm(2))[0], two, "the render in between")
    r.accum_add(4)
    _same(r.accum_read()[0], seven, "the accumulation around a render")
    r.accum_end()


def _raises(rt, code, fn, *a, **kw):
    with pytest.raises(rt.RtError, match=r"\(-%d\)" % code):
        fn(*a, **kw)


def test_state_and_arguments(rt, ctx):
    f = rt._ffi
    r = ctx
    bare = rt.Renderer(0)
    try:
        scene = _scenes.get("test_sphere") or rt.Scene.build("test_sphere", 2.0)
        _raises(rt, f.ERR_STATE, bare.accum_begin, scene.camera, rt.make_params(40, 20, 1))  # no scene
        _raises(rt, f.ERR_STATE, bare.render_to_noise, scene.camera, rt.make_params(40, 20, 4), 0.1, 2)
        _raises(rt, f.ERR_STATE, bare.accum_add, 1)
        bare.accum_end()  # nothing open: no error
    finally:
        bare.close()
    scene, prm = _setup(rt, r, "A")
    before = r.render(scene.camera, prm(2), want_rgb8=True)
    kept = [before[0].copy(), before[1].copy()]
    _raises(rt, f.ERR_STATE, r.accum_add, 1)
    _raises(rt, f.ERR_STATE, r.accum_read)
    r.accum_end()
    _raises(rt, f.ERR_INVALID, r.accum_begin, scene.camera, prm(0))
    # before the first add: zeros, no division by 0
    r.accum_begin(scene.camera, prm(1))
    img, rgb8, sem, noise = r.accum_read(want_rgb8=True, want_sem=True)
    assert img.shape == (20, 40, 3) and sem.shape == (20, 40) and not img.any() and not rgb8.any() and not sem.any()
    assert (noise.spp_done, noise.mean_luminance, noise.rms_sem, noise.noise) == (0, 0.0, 0.0, np.inf)
    _raises(rt, f.ERR_INVALID, r.accum_add, 0)
    r.accum_add(1)
    _same(r.accum_read()[0], r.render(scene.camera, prm(1))[0], "after the refused add")
    # the bound of spp holds for first_sample + everything added; the add that would pass it changes nothing
    r.accum_begin(scene.camera, prm(1), first_sample=2 ** 32 - 2)
    r.accum_add(1)
    last = r.accum_read()
    _raises(rt, f.ERR_INVALID, r.accum_add, 1)
    again = r.accum_read()
    assert again[3].spp_done == 1
    _same(again[0], last[0], "after the add past the bound")
    # rt_render_to_noise: its arguments, and an open accumulation
    for target, step, spp in ((0.1, 0, 8), (float("nan"), 4, 8), (-1.0, 4, 8), (0.1, 4, 1)):
        r.accum_end()
        _raises(rt, f.ERR_INVALID, r.render_to_noise, scene.camera, prm(spp), target, step)
    r.accum_begin(scene.camera, prm(1))
    _raises(rt, f.ERR_STATE, r.render_to_noise, scene.camera, prm(8), 0.1, 4)
    r.accum_add(1)  # (still open)
    # what ends an accumulation; none of them touches what rt_render gave and gives
    enders = [("upload", lambda: r.upload(scene)), ("set_lens", lambda: r.set_lens(None)), ("set_motion", lambda: r.set_motion(None)),
              ("set_quads", lambda: r.set_quads(None)), ("set_lights", lambda: r.set_lights(None)),
              ("set_option", lambda: r.set_option("chains", 0)), ("accum_end", r.accum_end)]
    for name, end in enders:
        r.accum_begin(scene.camera, prm(1))
        r.accum_add(1)
        end()
        _raises(rt, f.ERR_STATE, r.accum_add, 1)
        _raises(rt, f.ERR_STATE, r.accum_read)
        _same(before[0], kept[0], (name, "the earlier output"))
        _same(before[1], kept[1], (name, "the earlier rgb8 output"))
        after = r.render(scene.camera, prm(2), want_rgb8=True)
        _same(after[0], kept[0], (name, "rt_render afterwards"))
        _same(after[1], kept[1], (name, "rt_render afterwards, rgb8"))
    # a refused set leaves it open
    r.accum_begin(scene.camera, prm(1))
    _raises(rt, f.ERR_INVALID, r.set_lens, (-1.0, 1.0))
    r.accum_add(1)
    r.accum_end()


@pytest.mark.parametrize("case", ["A", "B", "D_lights"])
def test_accumulation_launches_the_production_kernels(rt, ctx, case):
    r = ctx
    tables = rt.variant_tables()
    assert [len(tables[k]) for k in ("shade", "intersect", "debug_bounce", "untabled")] == [66, 66, 15, 7]
    scene, prm = _setup(rt, r, case)
    r.launched_variants(reset=True)
    r.render(scene.camera, prm(7))
    frame = r.launched_variants(reset=True)
    assert frame["shade"] and not frame["debug_bounce"]
    r.accum_begin(scene.camera, prm(7))
    r.accum_add(7)
    r.accum_read(want_rgb8=True, want_sem=True)
    assert r.launched_variants(reset=True) == frame
    r.accum_end()
