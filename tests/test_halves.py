"""The half buffers on the GPU (rt_accum_track_halves, rt_accum_read_halves, rt_accum_denoise_halves, rt_accum_export_halves,
rt_accum_import_halves): the halves of rendered accumulations against the numpy accumulation of their single-sample frames by parity, bit
for bit; everything else an accumulation returns unchanged with tracking on; the cross filter, e_p and the frame figures on designed states
against tests/halves_ref.py, bit for bit; resume; the errors of the header; and the error of rendered frames against converged ones."""
import ctypes as C
import struct

import numpy as np
import pytest

import accum_state_ref
import denoise_ref
import halves_ref as ref
import noise_ref

pytestmark = pytest.mark.gpu

SEED = 1234
NX, NY = 20, 18


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()), "values differ")


def _held(got, want, what):
    """The same bits where the reference is a number, a NaN where it is one."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.where(np.isnan(want), ~np.isnan(got), _bits(got) != _bits(want)) if got.dtype.kind == "f" else got != want
    assert not bad.any(), (what, int(bad.sum()), "values differ, first at", tuple(int(i) for i in np.argwhere(bad)[0]))


def _figure_bits(x):
    return "nan" if x != x else struct.pack("<d", x).hex()


def _raises(rt, code, fn, *a, **kw):
    with pytest.raises(rt.RtError, match=r"\(-%d\)" % code):
        fn(*a, **kw)


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    yield r
    r.set_option("pixel_order", 0)
    r.close()


@pytest.fixture(scope="module")
def ctx2(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


_scenes, _single = {}, {}


def _scene(rt, name, aspect):
    if (name, aspect) not in _scenes:
        _scenes[name, aspect] = rt.Scene.build(name, aspect)
    return _scenes[name, aspect]


def _setup(rt, r, po=0, **shard):
    scene = _scene(rt, "test_sphere", NX / NY)
    r.set_option("pixel_order", po)
    r.upload(scene)
    return scene, lambda spp, **kw: rt.make_params(NX, NY, spp, **{"seed": SEED, "spp_slice": 2, "max_depth": 50, **shard, **kw})


def _singles(r, scene, prm, key, lo, hi):
    """x[i], lo <= i < hi: the frame of the sample with the absolute index i, from a one-sample accumulation each (sum = 0 + x_i); computed
    once and never changed."""
    have = _single.setdefault(key, {})
    for i in range(lo, hi):
        if i not in have:
            r.accum_begin(scene.camera, prm(1), first_sample=i)
            r.accum_add(1)
            img = r.accum_export().sum
            img.setflags(write=False)
            have[i] = img
    r.accum_end()
    return [have[i] for i in range(lo, hi)]


def _halves_are(rt, r, want, first, n, what, counts=None):
    """The exported halves and both half images against the reference split `want`."""
    got = r.accum_export_halves()
    assert (got.nx, got.rows, got.first_sample, got.done) == (want[0][0].shape[1], want[0][0].shape[0], first, n) and got.check()
    for h in range(2):
        _same(got.sum[h], want[h][0], (what, "sum", h))
        _same(got.moments[h][..., 0], want[h][1], (what, "S1", h))
        _same(got.moments[h][..., 1], want[h][2], (what, "S2", h))
        nh = ref.n_h(first, n if counts is None else counts, h)
        c, sem = ref.read_half(*want[h], nh)
        img, got_sem = r.accum_half(h, want_sem=True)
        _same(img, c, (what, "half image", h))
        _same(got_sem, sem, (what, "half sem", h))
    assert (want[0][0] != 0).any() and (want[1][0] != 0).any() and (want[0][0] != want[1][0]).any()


# ---- 1. the defining property -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 7])
def test_halves_are_the_in_order_sums_of_their_parity(rt, ctx, first):
    r = ctx
    scene, prm = _setup(rt, r)
    x = _singles(r, scene, prm, "full", first, first + 9)
    want = ref.split(x, first)
    r.accum_begin(scene.camera, prm(4), first_sample=first)
    r.accum_track_halves()
    done = 0
    for n in (3, 2, 4):  # slices of 2: the adds begin on both parities and end inside and on slice boundaries
        r.accum_add(n)
        done += n
        _halves_are(rt, r, ref.split(x[:done], first), first, done, (first, "after", done))
    if first == 0:
        _same(r.accum_read()[0], r.render(scene.camera, prm(9))[0], "the accumulation itself is rt_render(9)")
    # one add of 9, under both other pixel orders
    for po in (1, 2):
        scene, prm = _setup(rt, r, po)
        r.accum_begin(scene.camera, prm(9), first_sample=first)
        r.accum_track_halves()
        r.accum_add(9)
        _halves_are(rt, r, want, first, 9, (first, "one add, pixel order", po))
    r.accum_end()


@pytest.mark.parametrize("first", [0, 7])
def test_halves_on_a_shard(rt, ctx, first):
    r = ctx
    shard = dict(shard_count=2, shard_band=4, shard_id=1)
    scene, prm = _setup(rt, r, **shard)
    x = _singles(r, scene, prm, "shard", first, first + 9)
    assert x[0].shape[0] == r.shard_rows(prm(1)) < NY
    r.accum_begin(scene.camera, prm(4), first_sample=first)
    r.accum_track_halves()
    for n in (3, 2, 4):
        r.accum_add(n)
    _halves_are(rt, r, ref.split(x, first), first, 9, (first, "shard"))
    kept = r.accum_export_halves()
    _raises(rt, rt._ffi.ERR_UNSUPPORTED, r.accum_denoise_halves)
    _same(r.accum_export_halves().sum, kept.sum, "the shard after the refusal")
    r.accum_end()


# ---- 2. adaptive ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 7])
def test_halves_of_an_adaptive_accumulation(rt, ctx, first):
    """min_samples 3 and a tolerance from the reference alone — the median relative error of the pixels after three samples — so that
    the quiet pixels (the sky) stop at 3 while the others go on; both groups are asserted to be there."""
    r = ctx
    scene, prm = _setup(rt, r)
    x = _singles(r, scene, prm, "full", first, first + 9)
    _, s1, s2, _ = noise_ref.accumulate(x[:3])
    ybar, v = noise_ref.pixel_figures(s1, s2, 3)
    rel = np.sqrt(v) / np.maximum(ybar, 0.01)
    tol = float(np.median(rel[rel > 0]))
    want3 = v <= (tol * np.maximum(ybar, 0.01)) ** 2  # the criterion of "Adaptive sampling" at the first decision that can stop a pixel
    assert 10 <= want3.sum() <= want3.size - 10
    r.accum_begin(scene.camera, prm(3), first_sample=first)
    r.accum_track_halves()
    for n in (3, 2, 2):
        r.accum_add_adaptive(n, tol, 0.01, 3)
    counts = r.accum_counts()[0]
    print(f"first {first}: tolerance {tol!r}, counts {np.unique(counts, return_counts=True)}")
    assert set(np.unique(counts)) <= {3, 5, 7} and np.array_equal(counts == 3, want3) and (counts == 7).sum() >= 10
    _halves_are(rt, r, ref.split(x[:7], first, counts), first, 7, (first, "adaptive"), counts)
    uniform = ref.split(x[:3], first)  # a stopped pixel is the pixel of a uniform accumulation of 3 samples
    got = r.accum_export_halves()
    for h in range(2):
        _same(got.sum[h][counts == 3], uniform[h][0][counts == 3], (first, "stopped pixels", h))
    r.accum_end()


# ---- 3. nothing else moves --------------------------------------------------------------------------------------------------------------
def _everything(r):
    img, rgb8, sem, noise = r.accum_read(want_rgb8=True, want_sem=True)
    counts, info = r.accum_counts()
    st = r.accum_export()
    return [("f32", img), ("rgb8", rgb8), ("sem", sem), ("noise", bytes(noise)), ("counts", counts), ("info", bytes(info)),
            ("denoise", r.accum_denoise()[0]), ("denoise channels", r.accum_denoise_channels()[0]), ("channel sem", r.accum_channel_sem()),
            ("state sum", st.sum), ("state moments", st.moments), ("state channel moments", st.channel_moments), ("state counts", st.counts),
            ("state converged", st.converged), ("state scalars", repr((st.first_sample, st.done, st.planes, st.frame_id)).encode())]


@pytest.mark.parametrize("adaptive", [False, True])
def test_nothing_else_moves(rt, ctx, adaptive):
    r = ctx
    scene, prm = _setup(rt, r)
    runs, ledgers = [], []
    for track in (False, True):
        r.accum_begin(scene.camera, prm(4), first_sample=7)
        r.accum_track_channels()
        if track:
            r.accum_track_halves()
        r.launched_variants(reset=True)
        for n in (3, 2, 4):
            r.accum_add_adaptive(n, 0.3, 0.01, 3) if adaptive else r.accum_add(n)
        ledgers.append(r.launched_variants(reset=True))
        if track:  # the calls of this feature launch nothing of a ledger family
            r.accum_half(0, want_sem=True), r.accum_denoise_halves(want_rgb8=True, want_err=True)
            hs = r.accum_export_halves()
            led = r.launched_variants(reset=True)
            assert not any(led.values()), led
            assert hs.done == 9
        runs.append(_everything(r))
    r.accum_end()
    assert ledgers[0] == ledgers[1] and any(ledgers[0].values())
    assert [k for k, _ in runs[0]] == [k for k, _ in runs[1]]
    for (k, a), (_, b) in zip(*runs):
        if isinstance(a, bytes):
            assert a == b, k
        else:
            _same(a, b, k)


# ---- 4. the filter on designed states -------------------------------------------------------------------------------------------------
def _import_designed(rt, r, halves, first, done, counts=None, conv=None):
    """test_sphere at the frame's aspect, an accumulation with the state (sum = the sum of the halves) and the halves imported."""
    rows, nx = halves[0][1].shape
    scene = _scene(rt, "test_sphere", nx / rows)
    r.set_option("pixel_order", 0)
    r.upload(scene)
    prm = rt.make_params(nx, rows, 1, max_depth=8, seed=77)
    fid = rt.accum_frame_id(scene.camera, prm)
    with np.errstate(all="ignore"):
        total = (halves[0][0] + halves[1][0]).astype(np.float32)
        mom = np.stack([halves[0][1] + halves[1][1], halves[0][2] + halves[1][2]], -1)
    planes = accum_state_ref.COUNTS if counts is not None else 0
    st = rt.AccumState(nx, rows, first, done, planes, fid, sum=total, moments=mom, counts=counts, converged=conv)
    hs = rt.AccumHalves(nx, rows, first, done, fid, sum=np.stack([halves[0][0], halves[1][0]]),
                        moments=np.stack([np.stack([h[1], h[2]], -1) for h in halves]))
    assert st.check() and hs.check()
    r.accum_begin(scene.camera, prm, first_sample=first)
    r.accum_import(st)
    r.accum_import_halves(hs)
    return hs


def _filter_is_the_reference(rt, r, halves, first, done, radius, patch, strength, what, counts=None, conv=None):
    hs = _import_designed(rt, r, halves, first, done, counts, conv)
    want = ref.cross_filter(halves, first, done if counts is None else counts, radius, patch, strength)
    img, rgb8, err, res = r.accum_denoise_halves(radius, patch, strength, want_rgb8=True, want_err=True)
    got = (res.mean_luminance, res.residual_rms, res.residual_noise)
    print(f"{what}: figures {got!r}, the reference {want['residual']!r}, shares {want['shares']!r}")
    _held(img, want["out"], (what, "out"))
    _held(err, want["err"], (what, "err"))
    _same(rgb8, want["rgb8"], (what, "rgb8"))
    assert [_figure_bits(x) for x in got] == [_figure_bits(x) for x in want["residual"]], (what, got, want["residual"])
    back = r.accum_export_halves()  # read, not changed
    _same(back.sum, hs.sum, (what, "halves after the filter")), _same(back.moments, hs.moments, (what, "moments after the filter"))
    r.accum_end()
    return want


def test_filter_kernel_case_with_a_nan_an_inf_and_a_zero_variance_block(rt, ctx):
    want = _filter_is_the_reference(rt, ctx, ref.kernel_halves(37, 21), 0, 16, 5, 1, denoise_ref.KERNEL_CASE_STRENGTH, "kernel case")
    assert min(min(s) for s in want["shares"]) >= 0.10 and np.isnan(want["out"]).any() and np.isinf(want["out"]).any()


@pytest.mark.parametrize("nx,rows,radius,patch", [(37, 21, 5, 1), (37, 5, 10, 3), (1, 1, 5, 1)])
def test_filter_plain_halves(rt, ctx, nx, rows, radius, patch):
    want = _filter_is_the_reference(rt, ctx, ref.plain_halves(nx, rows), 3, 16, radius, patch, 0.45, ("plain", nx, rows))
    assert all(np.isfinite(want["residual"]))


@pytest.mark.parametrize("first", [4, 7])
def test_filter_adaptive_state_with_pixels_of_0_to_3_samples(rt, ctx, first):
    cnt, conv = ref.adaptive_counts(37, 21)
    want = _filter_is_the_reference(rt, ctx, ref.plain_halves(37, 21, nh=4), first, 8, 5, 1, 0.45, ("adaptive", first), cnt, conv)
    assert np.isnan(want["err"]).any() and np.isnan(want["residual"][1]) and np.isfinite(want["residual"][0])


def test_filter_more_than_256_partial_sums(rt, ctx):
    want = _filter_is_the_reference(rt, ctx, ref.extremes_halves(), 0, 16, 1, 0, 0.45, "257 x 256")
    assert int(np.argmax(want["err"])) > 65536


# ---- 5. resume --------------------------------------------------------------------------------------------------------------------------
def _halves_everything(r):
    out = []
    for h in range(2):
        img, sem = r.accum_half(h, want_sem=True)
        out += [(f"half {h}", img), (f"half sem {h}", sem)]
    img, rgb8, err, res = r.accum_denoise_halves(want_rgb8=True, want_err=True)
    hs = r.accum_export_halves()
    return out + [("cross", img), ("cross rgb8", rgb8), ("err", err), ("residual", bytes(res)), ("sum", hs.sum), ("moments", hs.moments)] + \
        [("read", r.accum_read()[0])]


def test_resume(rt, ctx, ctx2):
    r, r2 = ctx, ctx2
    scene, prm = _setup(rt, r)
    r.accum_begin(scene.camera, prm(5), first_sample=7)
    r.accum_track_halves()
    r.accum_add(5)
    st, hs = r.accum_export(), r.accum_export_halves()
    r.accum_add(4)
    want = _halves_everything(r)
    r.accum_end()
    r2.upload(scene)
    r2.accum_begin(scene.camera, prm(4), first_sample=7)
    r2.accum_import(st)
    r2.accum_import_halves(hs)
    _same(r2.accum_export_halves().sum, hs.sum, "an export straight after the import")
    r2.accum_add(4)
    got = _halves_everything(r2)
    r2.accum_end()
    for (k, a), (_, b) in zip(got, want):
        if isinstance(a, bytes):
            assert a == b, k
        else:
            _held(a, b, k)


def test_render_to_residual_stops_on_the_target_or_the_maximum(rt, ctx):
    r = ctx
    scene, prm = _setup(rt, r)
    r.accum_begin(scene.camera, prm(4))
    r.accum_track_halves()
    r.accum_add(4)
    at4 = r.accum_denoise_halves(want_err=True)
    r.accum_add(4), r.accum_add(4)
    at12 = r.accum_denoise_halves(want_err=True)
    r.accum_end()
    assert 0 < at12[3].residual_noise and 0 < at4[3].residual_noise
    img, _, err, res, done = r.render_to_residual(scene.camera, prm(12), at4[3].residual_noise, 4, want_err=True)  # met after the first step
    assert done == 4 and bytes(res) == bytes(at4[3])
    _same(img, at4[0], "stopped on the target"), _same(err, at4[2], "stopped on the target, err")
    img, _, _, res, done = r.render_to_residual(scene.camera, prm(12), 0.0, 4)  # never met: the maximum
    assert done == 12 and bytes(res) == bytes(at12[3])
    _same(img, at12[0], "stopped on the maximum")
    img, _, _, res, done = r.render_to_residual(scene.camera, prm(6), 0.0, 1)  # a step below 4: the first add still gives each half two samples
    assert done == 6
    _raises(rt, rt._ffi.ERR_STATE, r.accum_export_halves)  # the accumulation is ended
    with pytest.raises(ValueError):
        r.render_to_residual(scene.camera, prm(3), 0.1, 4)


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_accumulation_unchanged(rt, ctx):
    r, f = ctx, rt._ffi
    scene, prm = _setup(rt, r)
    r.accum_end()
    for fn in (r.accum_track_halves, lambda: r.accum_half(0), r.accum_denoise_halves, r.accum_export_halves):
        _raises(rt, f.ERR_STATE, fn)  # no accumulation
    r.accum_begin(scene.camera, prm(4))
    for fn in (lambda: r.accum_half(0), r.accum_denoise_halves, r.accum_export_halves):
        _raises(rt, f.ERR_STATE, fn)  # no tracking
    r.accum_add(1)
    _raises(rt, f.ERR_STATE, r.accum_track_halves)  # after an add
    fresh = rt.AccumHalves(NX, NY, 0, 1, rt.accum_frame_id(scene.camera, prm(1)))
    _raises(rt, f.ERR_STATE, r.accum_import_halves, fresh)  # after an add
    r.accum_begin(scene.camera, prm(4))
    r.accum_track_halves()
    r.accum_track_halves()  # a second call: RT_OK
    r.accum_track_channels()  # combines freely
    r.accum_add(3)
    kept = _everything(r), r.accum_export_halves()

    def unchanged(what):
        now = _everything(r), r.accum_export_halves()
        for (k, a), (_, b) in zip(now[0], kept[0]):
            assert a == b if isinstance(a, bytes) else np.array_equal(_bits(a), _bits(b)), (what, k)
        _same(now[1].sum, kept[1].sum, what), _same(now[1].moments, kept[1].moments, what)

    _raises(rt, f.ERR_STATE, r.accum_denoise_halves)  # three samples: a half holds one
    _raises(rt, f.ERR_INVALID, r.accum_half, 2)
    for bad in (dict(radius=0), dict(radius=f.DENOISE_MAX_RADIUS + 1), dict(patch=f.DENOISE_MAX_PATCH + 1), dict(strength=0.0), dict(strength=float("nan"))):
        _raises(rt, f.ERR_INVALID, r.accum_denoise_halves, **bad)
    st = r.accum_export()
    _raises(rt, f.ERR_UNSUPPORTED, r.accum_import, st)
    nxt = rt.AccumState(NX, NY, 3, 1, 0, st.frame_id, sum=st.sum, moments=st.moments)
    _raises(rt, f.ERR_UNSUPPORTED, r.accum_merge, nxt)
    _raises(rt, f.ERR_STATE, r.accum_import_halves, kept[1])  # after an add
    unchanged("after the refusals")
    r.accum_add(1)
    fp = C.POINTER(C.c_float)
    img = np.zeros((NY, NX, 3), np.float32)
    assert r._lib.rt_accum_denoise_halves(r._ctx, None, img.ctypes.data_as(fp), None, None, None) == 0  # NULL: the defaults, and NULL outputs
    _same(img, r.accum_denoise_halves(5, 1, f.DENOISE_HALVES_DEFAULT_STRENGTH)[0], "NULL against the explicit defaults")
    assert r._lib.rt_accum_read_halves(r._ctx, 1, None, None) == 0
    # the mismatches of an import
    good = r.accum_export_halves()
    r.accum_begin(scene.camera, prm(4))
    r.accum_import(rt.AccumState(NX, NY, 0, 4, 0, good.frame_id, sum=st.sum, moments=st.moments))
    for field, value in (("nx", NX + 1), ("rows", NY - 1), ("frame_id", good.frame_id ^ 1), ("first_sample", 1), ("done", 3)):
        bad = rt.AccumHalves(good.nx, good.rows, good.first_sample, good.done, good.frame_id, sum=good.sum, moments=good.moments)
        setattr(bad, field, value)
        rc = r._lib.rt_accum_import_halves(r._ctx, C.byref(bad.as_struct()))
        assert rc == -f.ERR_INVALID, (field, rc)
        _raises(rt, f.ERR_STATE, r.accum_export_halves)  # still not tracking: nothing changed
    hs = good.as_struct()
    hs.reserved[1] = 1
    assert r._lib.rt_accum_import_halves(r._ctx, C.byref(hs)) == -f.ERR_INVALID
    r.accum_import_halves(good)
    _same(r.accum_export_halves().sum, good.sum, "the import after the refusals")
    r.accum_track_halves()  # tracking already: RT_OK
    r.accum_end()
    # track_halves after an import that brought samples: their halves are unknown
    r.accum_begin(scene.camera, prm(4))
    r.accum_import(rt.AccumState(NX, NY, 0, 4, 0, good.frame_id, sum=st.sum, moments=st.moments))
    _raises(rt, f.ERR_STATE, r.accum_track_halves)
    r.accum_end()


# ---- 7. rendered frames -----------------------------------------------------------------------------------------------------------------
# cornell_box 64 x 64, depth 8, 16 spp, R 5, F 1, against rt_render at 4 096 spp with another seed (the two bit-reproducible frames of
# tests/test_denoise.py).  Measured on an MI355X, RMSE of the linear radiance:
#   with Scene.lights: 16 spp 0.17207, self-guided (strength 1.0) 0.07307; cross filter at 0.45 / 0.7 / 1.0: 0.09132 / 0.07848 / 0.07084
#   without          : 16 spp 0.25412, self-guided (strength 1.0) 0.08964; cross filter at 0.45 / 0.7 / 1.0: 0.10343 / 0.09295 / 0.09252
# RT_DENOISE_HALVES_DEFAULT_STRENGTH = 0.7: 1.0 is 9.7 % better with the lights and 0.5 % without, not "more than 5 % on both".
# MEASURED_RATIO = RMSE(cross filter at the default) / RMSE(16 spp); the bound is its geometric mean with 1, as in tests/test_denoise.py.
# MEASURED_G = residual_rms / (true luminance RMSE of out) at the default: 0.05611 / 0.07683 and 0.05856 / 0.09081.  The frames are
# reproducible; the factor sqrt(2) only keeps the test alive when the reference frame is regenerated.
MEASURED_RATIO = {"lights": 0.4561, "no_lights": 0.3658}
MEASURED_G = {"lights": 0.7304, "no_lights": 0.6449}
_truth = {}


def _lum_rmse(a, b):
    d = ref.lum32(a).astype(np.float64) - ref.lum32(b).astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


@pytest.mark.parametrize("which", ["lights", "no_lights"])
def test_rendered_frames(rt, ctx, which):
    r = ctx
    scene = _scene(rt, "cornell_box", 1.0)
    r.set_option("pixel_order", 0)
    r.upload(scene)
    if which == "lights":
        r.set_lights(scene.lights)
    if which not in _truth:
        _truth[which] = r.render(scene.camera, rt.make_params(64, 64, 4096, max_depth=8, seed=SEED + 1))[0]
    truth = _truth[which]
    r.accum_begin(scene.camera, rt.make_params(64, 64, 16, max_depth=8, seed=SEED))
    r.accum_track_halves()
    r.accum_add(16)
    noisy = r.accum_read()[0]
    e_noisy, e_self = denoise_ref.rmse(noisy, truth), denoise_ref.rmse(r.accum_denoise()[0], truth)
    for k in (0.45, 0.7, 1.0):
        img, _, _, res = r.accum_denoise_halves(strength=k)
        print(f"{which}: strength {k}: RMSE 16 spp {e_noisy:.5f}, self-guided {e_self:.5f}, cross {denoise_ref.rmse(img, truth):.5f}, "
              f"ratio {denoise_ref.rmse(img, truth) / e_noisy:.4f}, residual_rms {res.residual_rms:.5f}, true luminance RMSE {_lum_rmse(img, truth):.5f}, "
              f"g {res.residual_rms / _lum_rmse(img, truth):.4f}")
    img, _, _, res = r.accum_denoise_halves()
    r.accum_end()
    r.set_lights(None)
    assert np.isfinite(img).all()
    g = res.residual_rms / _lum_rmse(img, truth)
    assert denoise_ref.rmse(img, truth) <= e_noisy * np.sqrt(MEASURED_RATIO[which])
    assert MEASURED_G[which] / np.sqrt(2) <= g <= MEASURED_G[which] * np.sqrt(2)
