"""The sample buckets on the GPU (rt_accum_track_buckets, rt_accum_read_robust, rt_accum_denoise_robust, rt_accum_export_buckets,
rt_accum_import_buckets): the buckets of rendered accumulations against the numpy accumulation of their single-sample frames by index modulo
M, bit for bit; everything else an accumulation returns unchanged with tracking on; the robust read-out, its trims and frame figures and the
filter on robust colours on designed states against tests/robust_ref.py, bit for bit; resume; the errors of the header; and the error of
rendered frames against converged ones."""
import ctypes as C
import struct

import numpy as np
import pytest

import accum_state_ref
import denoise_ref
import noise_ref
import robust_ref as ref

pytestmark = pytest.mark.gpu

SEED = 1234
NX, NY = 20, 18
MODES = {"gini": ref.GINI, "median": ref.MEDIAN, "trim": ref.TRIM}


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
    return x if isinstance(x, int) else "nan" if x != x else struct.pack("<d", x).hex()


def _info(i):
    return (i.mean_luminance_plain, i.mean_luminance_robust, i.energy_removed, i.trimmed_fraction, int(i.nonfinite_dropped))


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


def _setup(rt, r, po=0, **kw0):
    scene = _scene(rt, "test_sphere", NX / NY)
    r.set_option("pixel_order", po)
    r.upload(scene)
    return scene, lambda spp, **kw: rt.make_params(NX, NY, spp, **{"seed": SEED, "spp_slice": 2, "max_depth": 50, **kw0, **kw})


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


def _buckets_are(r, want, first, n, what):
    """The exported buckets against the reference split `want` [M, rows, nx, 3]."""
    got = r.accum_export_buckets()
    assert (got.nx, got.rows, got.first_sample, got.done, got.M) == (want.shape[2], want.shape[1], first, n, want.shape[0]) and got.check(), what
    _same(got.sum, want, (what, "bucket sums"))
    assert (want != 0).any()
    return got


# ---- 1. the defining property -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 7])
@pytest.mark.parametrize("M", [3, 5])
def test_buckets_are_the_in_order_sums_of_their_index_class(rt, ctx, M, first):
    r = ctx
    scene, prm = _setup(rt, r)
    x = _singles(r, scene, prm, "full", first, first + 10)
    r.accum_begin(scene.camera, prm(4), first_sample=first)
    r.accum_track_buckets(M)
    done = 0
    for n in (3, 2, 4, 1):  # slices of 2: the adds begin and end inside a bucket cycle, inside and on slice boundaries; n < M after the first for M = 5
        r.accum_add(n)
        done += n
        got = _buckets_are(r, ref.split(x[:done], first, M), first, done, (M, first, "after", done))
        want = ref.read(got.sum, noise_ref.accumulate(x[:done])[0], first, done)
        img, info, trim = r.accum_robust(want_trim=True)
        _held(img, want["out"], (M, first, done, "robust image")), _same(trim, want["trim"], (M, first, done, "trim"))
    if first == 0:
        _same(r.accum_read()[0], r.render(scene.camera, prm(10))[0], "the accumulation itself is rt_render(10)")
    want = ref.split(x, first, M)
    for po in (1, 2):  # one add of 10, under both other pixel orders
        scene, prm = _setup(rt, r, po)
        r.accum_begin(scene.camera, prm(10), first_sample=first)
        r.accum_track_buckets(M)
        r.accum_add(10)
        _buckets_are(r, want, first, 10, (M, first, "one add, pixel order", po))
    r.accum_end()


@pytest.mark.parametrize("first", [0, 7])
def test_sixteen_buckets_of_five_samples_and_a_slice_longer_than_a_cycle(rt, ctx, first):
    r = ctx
    scene, prm = _setup(rt, r)
    x = _singles(r, scene, prm, "full", first, first + 10)
    r.accum_begin(scene.camera, prm(5), first_sample=first)
    r.accum_track_buckets(16)
    r.accum_add(5)
    got = _buckets_are(r, ref.split(x[:5], first, 16), first, 5, (first, "M 16, 5 samples"))
    assert sum(1 for b in range(16) if not got.sum[b].any()) == 11  # eleven empty buckets
    want = ref.read(got.sum, noise_ref.accumulate(x[:5])[0], first, 5, ref.MEDIAN)
    img, info, trim = r.accum_robust("median", want_trim=True)
    _held(img, want["out"], "M 16 median"), _same(trim, want["trim"], "M 16 trim")
    assert (trim == 2).all() and _info(info)[4] == 0  # K = 5: the empty buckets are not means, and not dropped ones
    # spp_slice 7, M 5: a slice is longer than a cycle and no multiple of it (slices of 7 and 3)
    scene, prm = _setup(rt, r, spp_slice=7)
    r.accum_begin(scene.camera, prm(10), first_sample=first)
    r.accum_track_buckets(5)
    r.accum_add(10)
    _buckets_are(r, ref.split(x, first, 5), first, 10, (first, "slices of 7"))
    r.accum_end()


@pytest.mark.parametrize("shard_id", [0, 1, 2])
def test_buckets_on_a_shard(rt, ctx, shard_id):
    r, first = ctx, 7
    shard = dict(shard_count=3, shard_band=2, shard_id=shard_id)
    scene, prm = _setup(rt, r, **shard)
    x = _singles(r, scene, prm, ("shard", shard_id), first, first + 10)
    assert x[0].shape[0] == r.shard_rows(prm(1)) < NY
    r.accum_begin(scene.camera, prm(4), first_sample=first)
    r.accum_track_buckets(5)
    for n in (3, 2, 4, 1):
        r.accum_add(n)
    got = _buckets_are(r, ref.split(x, first, 5), first, 10, ("shard", shard_id))
    want = ref.read(got.sum, noise_ref.accumulate(x)[0], first, 10)
    img, info, trim, rgb8 = r.accum_robust(want_trim=True, want_rgb8=True)  # the read-out works on shards
    _held(img, want["out"], "shard image"), _same(trim, want["trim"], "shard trim"), _same(rgb8, want["rgb8"], "shard rgb8")
    assert [_figure_bits(v) for v in _info(info)] == [_figure_bits(v) for v in want["info"]]
    _raises(rt, rt._ffi.ERR_UNSUPPORTED, r.accum_denoise_robust)
    _same(r.accum_export_buckets().sum, got.sum, "the shard after the refusal")
    r.accum_end()


@pytest.mark.parametrize("first", [0, 7])
def test_buckets_of_an_adaptive_accumulation(rt, ctx, first):
    """min_samples 3 and a tolerance from the reference alone — the median relative error of the pixels after three samples — so that the
    quiet pixels stop at 3 while the others go on; both groups are asserted to be there."""
    r = ctx
    scene, prm = _setup(rt, r)
    x = _singles(r, scene, prm, "full", first, first + 10)
    _, s1, s2, _ = noise_ref.accumulate(x[:3])
    ybar, v = noise_ref.pixel_figures(s1, s2, 3)
    rel = np.sqrt(v) / np.maximum(ybar, 0.01)
    tol = float(np.median(rel[rel > 0]))
    want3 = v <= (tol * np.maximum(ybar, 0.01)) ** 2
    assert 10 <= want3.sum() <= want3.size - 10
    r.accum_begin(scene.camera, prm(3), first_sample=first)
    r.accum_track_buckets(5)
    for n in (3, 2, 2):
        r.accum_add_adaptive(n, tol, 0.01, 3)
    counts = r.accum_counts()[0]
    assert set(np.unique(counts)) <= {3, 5, 7} and np.array_equal(counts == 3, want3) and (counts == 7).sum() >= 10
    got = _buckets_are(r, ref.split(x[:7], first, 5, counts), first, 7, (first, "adaptive"))
    total = r.accum_export().sum
    for mode in MODES:
        want = ref.read(got.sum, total, first, counts, MODES[mode], 1)
        img, info, trim = r.accum_robust(mode, 1, want_trim=True)
        _held(img, want["out"], (first, mode, "adaptive image")), _same(trim, want["trim"], (first, mode, "adaptive trim"))
        assert [_figure_bits(v) for v in _info(info)] == [_figure_bits(v) for v in want["info"]]
    r.accum_end()


# ---- 2. nothing else moves --------------------------------------------------------------------------------------------------------------
def _everything(r):
    img, rgb8, sem, noise = r.accum_read(want_rgb8=True, want_sem=True)
    counts, info = r.accum_counts()
    st, hs = r.accum_export(), r.accum_export_halves()
    out = [("f32", img), ("rgb8", rgb8), ("sem", sem), ("noise", bytes(noise)), ("counts", counts), ("info", bytes(info)),
           ("denoise", r.accum_denoise()[0]), ("denoise channels", r.accum_denoise_channels()[0]), ("channel sem", r.accum_channel_sem()),
           ("state sum", st.sum), ("state moments", st.moments), ("state channel moments", st.channel_moments), ("state counts", st.counts),
           ("state converged", st.converged), ("state scalars", repr((st.first_sample, st.done, st.planes, st.frame_id)).encode()),
           ("halves sum", hs.sum), ("halves moments", hs.moments)]
    for h in range(2):
        a, b = r.accum_half(h, want_sem=True)
        out += [(f"half {h}", a), (f"half sem {h}", b)]
    if st.done >= 4:
        img, rgb8, err, res = r.accum_denoise_halves(want_rgb8=True, want_err=True)
        out += [("cross", img), ("cross rgb8", rgb8), ("cross err", err), ("residual", bytes(res))]
    return out


@pytest.mark.parametrize("adaptive", [False, True])
def test_nothing_else_moves(rt, ctx, adaptive):
    r = ctx
    scene, prm = _setup(rt, r)
    runs, ledgers = [], []
    for track in (False, True):
        r.accum_begin(scene.camera, prm(4), first_sample=7)
        r.accum_track_channels()
        r.accum_track_halves()
        if track:
            r.accum_track_buckets(5)
        r.launched_variants(reset=True)
        for n in (3, 2, 4):
            r.accum_add_adaptive(n, 0.3, 0.01, 3) if adaptive else r.accum_add(n)
        ledgers.append(r.launched_variants(reset=True))
        if track:  # the calls of this feature launch nothing of a ledger family
            r.accum_robust(want_trim=True, want_rgb8=True), r.accum_denoise_robust(want_rgb8=True)
            bs = r.accum_export_buckets()
            led = r.launched_variants(reset=True)
            assert not any(led.values()), led
            assert bs.done == 9 and bs.M == 5
        runs.append(_everything(r))
    r.accum_end()
    assert ledgers[0] == ledgers[1] and any(ledgers[0].values())
    assert [k for k, _ in runs[0]] == [k for k, _ in runs[1]]
    for (k, a), (_, b) in zip(*runs):
        if isinstance(a, bytes):
            assert a == b, k
        else:
            _same(a, b, k)


# ---- 3. the read-out on designed states -----------------------------------------------------------------------------------------------
_designed = {}


def _designed_state(key, make):
    if key not in _designed:
        buckets, total, first, done, cnt, conv = make()
        s1, s2 = ref.designed_moments(total, done)
        for a in (buckets, total, s1, s2):
            a.setflags(write=False)
        _designed[key] = (buckets, total, first, done, cnt, conv, s1, s2)
    return _designed[key]


def _import_designed(rt, r, state):
    """test_sphere at the frame's aspect, an accumulation with the state and the buckets imported."""
    buckets, total, first, done, cnt, conv, s1, s2 = state
    M, rows, nx = buckets.shape[:3]
    scene = _scene(rt, "test_sphere", nx / rows)
    r.set_option("pixel_order", 0)
    r.upload(scene)
    prm = rt.make_params(nx, rows, 1, max_depth=8, seed=77)
    fid = rt.accum_frame_id(scene.camera, prm)
    st = rt.AccumState(nx, rows, first, done, accum_state_ref.COUNTS if cnt is not None else 0, fid, sum=total, moments=np.stack([s1, s2], -1), counts=cnt,
                       converged=conv)
    bs = rt.AccumBuckets(nx, rows, M, first, done, fid, sum=buckets)
    assert st.check() and bs.check()
    r.accum_begin(scene.camera, prm, first_sample=first)
    r.accum_import(st)
    r.accum_import_buckets(bs)
    return bs


def _readout_is_the_reference(rt, r, state, what, modes=(("gini", 0), ("median", 0), ("trim", 0), ("trim", 1), ("trim", 100))):
    buckets, total, first, done, cnt = state[:5]
    bs = _import_designed(rt, r, state)
    wants = {}
    for mode, trim in modes:
        want = wants[mode, trim] = ref.read(buckets, total, first, done if cnt is None else cnt, MODES[mode], trim)
        img, info, t, rgb8 = r.accum_robust(mode, trim, want_trim=True, want_rgb8=True)
        print(f"{what} {mode} {trim}: figures {_info(info)!r}, the reference {want['info']!r}")
        _held(img, want["out"], (what, mode, trim, "out"))
        _same(t, want["trim"], (what, mode, trim, "trim"))
        _same(rgb8, want["rgb8"], (what, mode, trim, "rgb8"))
        assert [_figure_bits(v) for v in _info(info)] == [_figure_bits(v) for v in want["info"]], (what, mode, trim, _info(info), want["info"])
    _same(r.accum_export_buckets().sum, bs.sum, (what, "buckets after the read-outs"))  # read, not changed
    r.accum_end()
    return wants


@pytest.mark.parametrize("first", [0, 7])
@pytest.mark.parametrize("K", [5, 16])
def test_readout_on_designed_means(rt, ctx, K, first):
    """The trim thresholds of GINI from both sides, one, two and (K + 1) / 2 firefly buckets, NaN, +inf and -inf buckets, all non-finite,
    zero and negative sums, -0.0, ties (robust_ref.designed_columns), on a 37 x 21 frame, all three modes, trim 0, 1 and 100."""
    state = _designed_state(("means", K, first), lambda: ref.designed_state(K, 37, 21, first))
    wants = _readout_is_the_reference(rt, ctx, state, ("means", K, first))
    g = wants["gini", 0]
    assert {0, 1, 2} <= set(np.unique(g["trim"])) and np.isnan(g["out"]).any() and g["info"][4] > 10
    _same(wants["trim", 100]["out"], wants["median", 0]["out"], "trim 100 is the median")


@pytest.mark.parametrize("K", [5, 16])
def test_readout_on_an_adaptive_state_with_counts_0_to_M_plus_1(rt, ctx, K):
    state = _designed_state(("counts", K), lambda: ref.designed_state(K, 37, 21, 7, counts=True))
    wants = _readout_is_the_reference(rt, ctx, state, ("counts", K), (("gini", 0), ("median", 0), ("trim", 1)))
    assert np.isnan(wants["gini", 0]["out"][state[4] == 0]).all()


def test_readout_with_more_than_256_partial_sums(rt, ctx):
    state = _designed_state("big", ref.big_state)
    wants = _readout_is_the_reference(rt, ctx, state, "257 x 256", (("gini", 0), ("median", 0)))
    assert all(np.isfinite(wants["gini", 0]["info"][:4])) and int((wants["gini", 0]["trim"] > 0).sum()) == 3


# ---- 4. the filter on robust colours ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,patch", [(5, 1), (2, 0)])
def test_denoise_robust_is_the_filter_on_the_robust_colours(rt, ctx, radius, patch):
    r = ctx
    state = _designed_state(("means", 5, 7), lambda: ref.designed_state(5, 37, 21, 7))
    buckets, total, first, done, _, _, s1, s2 = state
    _import_designed(rt, r, state)
    for mode, strength in (("gini", 0.45), ("median", 1.0)):
        want = ref.denoise_robust(buckets, total, s1, s2, first, done, radius, patch, strength, MODES[mode])
        img, rgb8 = r.accum_denoise_robust(mode, 0, radius, patch, strength, want_rgb8=True)
        _held(img, want["out"], (radius, patch, mode, "out")), _same(rgb8, want["rgb8"], (radius, patch, mode, "rgb8"))
        assert (strength != 0.45 or min(want["shares"]) > 0.05) and np.isnan(want["colours"]).any() and np.isfinite(want["colours"]).mean() > 0.99
    plain = r.accum_denoise(radius, patch, 0.45)[0]  # the unchanged filter still reads the plain colours
    with np.errstate(all="ignore"):
        ybar, v = noise_ref.pixel_figures(s1, s2, done)
        _held(plain, denoise_ref.denoise(ref.plain(total, done), ybar.astype(np.float32), v.astype(np.float32), radius, patch, 0.45)[0], "rt_accum_denoise beside it")
    r.accum_end()


# ---- 5. resume --------------------------------------------------------------------------------------------------------------------------
def _robust_everything(r):
    out = []
    for mode in MODES:
        img, info, trim, rgb8 = r.accum_robust(mode, 1, want_trim=True, want_rgb8=True)
        out += [(mode, img), (mode + " info", bytes(info)), (mode + " trim", trim), (mode + " rgb8", rgb8)]
    img, rgb8 = r.accum_denoise_robust(want_rgb8=True)
    bs, hs = r.accum_export_buckets(), r.accum_export_halves()
    return out + [("filtered", img), ("filtered rgb8", rgb8), ("buckets", bs.sum), ("halves", hs.sum), ("read", r.accum_read()[0]),
                  ("cross", r.accum_denoise_halves()[0])]


def test_resume(rt, ctx, ctx2):
    r, r2 = ctx, ctx2
    scene, prm = _setup(rt, r)
    r.accum_begin(scene.camera, prm(5), first_sample=7)
    r.accum_track_halves(), r.accum_track_buckets(5)
    r.accum_add(4)
    st, hs, bs = r.accum_export(), r.accum_export_halves(), r.accum_export_buckets()
    r.accum_add(5)
    want = _robust_everything(r)
    r.accum_end()
    r2.upload(scene)
    r2.accum_begin(scene.camera, prm(4), first_sample=7)
    r2.accum_import(st), r2.accum_import_halves(hs), r2.accum_import_buckets(bs)
    _same(r2.accum_export_buckets().sum, bs.sum, "an export straight after the import")
    r2.accum_add(5)
    got = _robust_everything(r2)
    r2.accum_end()
    for (k, a), (_, b) in zip(got, want):
        if isinstance(a, bytes):
            assert a == b, k
        else:
            _held(a, b, k)


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_accumulation_unchanged(rt, ctx):
    r, f = ctx, rt._ffi
    scene, prm = _setup(rt, r)
    r.accum_end()
    for fn in (lambda: r.accum_track_buckets(5), r.accum_robust, r.accum_denoise_robust, r.accum_export_buckets):
        _raises(rt, f.ERR_STATE, fn)  # no accumulation
    r.accum_begin(scene.camera, prm(4))
    for fn in (r.accum_robust, r.accum_denoise_robust, r.accum_export_buckets):
        _raises(rt, f.ERR_STATE, fn)  # no tracking
    for M in (0, 2, 17):
        _raises(rt, f.ERR_INVALID, r.accum_track_buckets, M)
    _raises(rt, f.ERR_STATE, r.accum_export_buckets)  # still not tracking
    r.accum_add(1)
    _raises(rt, f.ERR_STATE, r.accum_track_buckets, 5)  # after an add
    fresh = rt.AccumBuckets(NX, NY, 5, 0, 1, rt.accum_frame_id(scene.camera, prm(1)))
    _raises(rt, f.ERR_STATE, r.accum_import_buckets, fresh)  # after an add
    r.accum_begin(scene.camera, prm(4))
    r.accum_track_buckets(5)
    r.accum_track_buckets(5)  # a second call with the same M: RT_OK
    _raises(rt, f.ERR_STATE, r.accum_track_buckets, 6)  # with another M
    r.accum_track_channels(), r.accum_track_halves()  # combines freely
    _raises(rt, f.ERR_STATE, r.accum_robust)  # fewer than 1 sample
    r.accum_add(1)
    _raises(rt, f.ERR_STATE, r.accum_denoise_robust)  # one sample: no variance
    r.accum_robust()
    r.accum_add(3)
    kept = _everything(r), r.accum_export_buckets(), _robust_everything(r)

    def unchanged(what):
        now = _everything(r), r.accum_export_buckets(), _robust_everything(r)
        for k in (0, 2):
            for (name, a), (_, b) in zip(now[k], kept[k]):
                assert a == b if isinstance(a, bytes) else np.array_equal(_bits(a), _bits(b)), (what, name)
        _same(now[1].sum, kept[1].sum, what)
        assert (now[1].M, now[1].done) == (5, 4)

    _raises(rt, f.ERR_STATE, r.accum_track_buckets, 6)
    _raises(rt, f.ERR_INVALID, r.accum_robust, 3)
    _raises(rt, f.ERR_INVALID, r.accum_denoise_robust, 3)
    rb = f.RtRobust(f.ROBUST_GINI, 0)
    rb.reserved[1] = 1
    assert r._lib.rt_accum_read_robust(r._ctx, C.byref(rb), None, None, None, None) == -f.ERR_INVALID
    assert r._lib.rt_accum_denoise_robust(r._ctx, C.byref(rb), None, None, None) == -f.ERR_INVALID
    for bad in (dict(radius=0), dict(radius=f.DENOISE_MAX_RADIUS + 1), dict(patch=f.DENOISE_MAX_PATCH + 1), dict(strength=0.0), dict(strength=float("nan"))):
        _raises(rt, f.ERR_INVALID, r.accum_denoise_robust, **bad)
    st = r.accum_export()
    _raises(rt, f.ERR_UNSUPPORTED, r.accum_import, st)
    nxt = rt.AccumState(NX, NY, 4, 1, f.ACCUM_STATE_CHANNELS, st.frame_id, sum=st.sum, moments=st.moments, channel_moments=st.channel_moments)
    _raises(rt, f.ERR_UNSUPPORTED, r.accum_merge, nxt)
    _raises(rt, f.ERR_STATE, r.accum_import_buckets, kept[1])  # after an add
    unchanged("after the refusals")
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    img = np.zeros((NY, NX, 3), np.float32)
    assert r._lib.rt_accum_read_robust(r._ctx, None, img.ctypes.data_as(fp), None, None, None) == 0  # NULL: GINI, and NULL outputs
    _same(img, r.accum_robust("gini")[0], "NULL against the explicit default")
    assert r._lib.rt_accum_read_robust(r._ctx, None, None, None, None, None) == 0
    assert r._lib.rt_accum_denoise_robust(r._ctx, None, None, img.ctypes.data_as(fp), None) == 0
    _same(img, r.accum_denoise_robust("gini", 0, 5, 1, f.DENOISE_DEFAULT_STRENGTH)[0], "NULL against the explicit defaults")
    # the mismatches of an import
    good = r.accum_export_buckets()
    plain_state = rt.AccumState(NX, NY, 0, 4, 0, good.frame_id, sum=st.sum, moments=st.moments)
    r.accum_begin(scene.camera, prm(4))
    r.accum_import(plain_state)
    for field, value in (("nx", NX + 1), ("rows", NY - 1), ("frame_id", good.frame_id ^ 1), ("first_sample", 1), ("done", 3)):
        bad = rt.AccumBuckets(good.nx, good.rows, good.M, good.first_sample, good.done, good.frame_id, sum=good.sum)
        setattr(bad, field, value)
        rc = r._lib.rt_accum_import_buckets(r._ctx, C.byref(bad.as_struct()))
        assert rc == -f.ERR_INVALID, (field, rc)
        _raises(rt, f.ERR_STATE, r.accum_export_buckets)  # still not tracking: nothing changed
    bs = good.as_struct()
    bs.reserved = 1
    assert r._lib.rt_accum_import_buckets(r._ctx, C.byref(bs)) == -f.ERR_INVALID
    r.accum_import_buckets(good)
    _same(r.accum_export_buckets().sum, good.sum, "the import after the refusals")
    r.accum_track_buckets(5)  # tracking already, the same M: RT_OK
    six = rt.AccumBuckets(NX, NY, 6, 0, 4, good.frame_id)
    _raises(rt, f.ERR_INVALID, r.accum_import_buckets, six)  # another M than the accumulation tracks
    _same(r.accum_export_buckets().sum, good.sum, "after the refused M")
    r.accum_end()
    # track_buckets after an import that brought samples: their buckets are unknown
    r.accum_begin(scene.camera, prm(4))
    r.accum_import(plain_state)
    _raises(rt, f.ERR_STATE, r.accum_track_buckets, 5)
    r.accum_end()
    _raises(rt, f.ERR_STATE, r.accum_robust)  # tracking ended with the accumulation
    # rt_accum_import and rt_accum_merge on an accumulation that tracks buckets (and nothing else)
    r.accum_begin(scene.camera, prm(4))
    r.accum_track_buckets(3)
    _raises(rt, f.ERR_UNSUPPORTED, r.accum_import, plain_state)
    r.accum_add(4)
    before = r.accum_export_buckets()
    _raises(rt, f.ERR_UNSUPPORTED, r.accum_import, plain_state)
    _raises(rt, f.ERR_UNSUPPORTED, r.accum_merge, rt.AccumState(NX, NY, 4, 1, 0, good.frame_id, sum=st.sum, moments=st.moments))
    _same(r.accum_export_buckets().sum, before.sum, "after the refused import and merge")
    assert r.accum_export().done == 4
    r.accum_begin(scene.camera, prm(4))
    _raises(rt, f.ERR_STATE, r.accum_export_buckets)  # and a new one does not track
    r.accum_end()


# ---- 7. rendered frames -----------------------------------------------------------------------------------------------------------------
# cornell_box 64 x 64, depth 8, 16 spp, M = 5, against rt_render at 4 096 spp with another seed (the two bit-reproducible frames of
# tests/test_denoise.py).  Measured on an MI355X, RMSE of the linear radiance:
#   with Scene.lights: plain mean 0.17207, GINI 0.17954 (ratio 1.0434), MEDIAN 0.20624; energy removed 6.3 %
#   without          : plain mean 0.25412, GINI 0.29829 (ratio 1.1738), MEDIAN 0.34766; energy removed 22.3 %
# The robust read-out is WORSE than the plain mean on both: at 16 spp every pixel of these frames is heavy-tailed and a bucket holds three
# samples, so the trim removes energy that belongs there.  MEASURED_RATIO = RMSE(GINI) / RMSE(plain).  The frames are reproducible; the
# factor sqrt(2) either way only keeps the test alive when the reference frame is regenerated.
MEASURED_RATIO = {"lights": 1.0434, "no_lights": 1.1738}
_truth = {}


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
    r.accum_track_buckets(5)
    r.accum_add(16)
    plain = r.accum_read()[0]
    img, info = r.accum_robust()
    r.accum_end()
    r.set_lights(None)
    e_plain, e_gini = denoise_ref.rmse(plain, truth), denoise_ref.rmse(img, truth)
    print(f"{which}: RMSE 16 spp plain {e_plain:.5f}, GINI {e_gini:.5f}, ratio {e_gini / e_plain:.4f}, energy removed {info.energy_removed:.4f}, "
          f"trimmed fraction {info.trimmed_fraction:.4f}")
    assert np.isfinite(img).all()
    assert MEASURED_RATIO[which] / np.sqrt(2) <= e_gini / e_plain <= MEASURED_RATIO[which] * np.sqrt(2)
