"""The read-out kernels of an accumulation on designed imported states (tests/designed_states.py): k_finalize<COUNTS>, k_sem<COUNTS>,
k_noise_partials<COUNTS> / k_noise_final<COUNTS>, k_adaptive_decide and k_adaptive_info, k_denoise_inputs<COUNTS>,
k_denoise_inputs_channels, k_channel_sem and, behind them, the two filters.  A state is built in numpy, imported right after
rt_accum_begin and read; nothing is traced except in the decision test (one sample on 24 x 16).  The scene, test_sphere, is uploaded only
so that rt_accum_begin succeeds.

Everything is held bit for bit.  Planes that travel (import -> export) are compared as bits, NaN payloads included.  Values the device
COMPUTES are compared as bits wherever the reference is a number, and as "a NaN too" where it is a NaN: IEEE 754 leaves the sign and
payload of a NaN an operation produces or passes on to the implementation, and numpy on x86 (inf - inf = the negative quiet NaN, the
first operand's payload) and gfx950 (the positive one) decide differently.  The frame figures are held bit for bit to
tests/noise_tree_ref.py, which adds over the kernels' tree in the accumulation's local pixel order, and — where every term is finite and
non-negative — to math.fsum within the analytic bound of that tree (noise_tree_ref.figure_bound)."""
import struct

import numpy as np
import pytest

import accum_state_ref as ref
import adaptive_ref
import denoise_channels_ref
import denoise_ref
import designed_states as ds
import frame_cases
import noise_tree_ref as tree

pytestmark = pytest.mark.gpu

SMALL_FRAMES = ((40, 20), (37, 21))      # 8 x 8 tiles plus four row-major rows; row-major
BIG_FRAMES = ((257, 256), (264, 250))    # 257 partial sums, row-major; 258: 248 rows in tiles plus 2 row-major (under RT_OPT_PIXEL_ORDER 2)
TOLERANCE, FLOOR = 0.05, 0.01


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()), "values differ")


def _held(got, want, what, where=None):
    """A computed plane against its reference: the same bits where the reference is a number, a NaN where it is one.  A failure names
    the classes of the state that hold a wrong pixel."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.where(np.isnan(want), ~np.isnan(got), _bits(got) != _bits(want)) if got.dtype.kind == "f" else got != want
    if bad.any():
        px = bad.any(axis=-1) if bad.ndim == 3 else bad
        classes = sorted(k for k, m in (where or {}).items() if (m & px).any())
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        assert False, (what, int(bad.sum()), "values differ, in the classes", classes, "first at", first, got[first], want[first])


def _figure_bits(x):
    return "nan" if x != x else struct.pack("<d", x).hex()


def _figures_are(noise, want, spp_done, what):
    got = (noise.mean_luminance, noise.rms_sem, noise.noise)
    print(f"{what}: figures {got!r}, the tree {want!r}")
    assert [_figure_bits(x) for x in got] == [_figure_bits(x) for x in want], (what, got, want)
    assert noise.spp_done == spp_done, (what, noise.spp_done, spp_done)


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    yield r
    r.set_option("pixel_order", 0)
    r.close()


_scenes, _orders = {}, {}


def _begin(rt, r, nx, rows, po=0):
    """Uploads test_sphere at the frame's aspect under RT_OPT_PIXEL_ORDER `po`; returns (camera, params, frame id, local index [rows, nx])."""
    if (nx, rows) not in _scenes:
        _scenes[nx, rows] = rt.Scene.build("test_sphere", nx / rows)
    scene = _scenes[nx, rows]
    r.set_option("pixel_order", po)
    r.upload(scene)
    prm = rt.make_params(nx, rows, 1, max_depth=8, seed=77)
    if (nx, rows, po) not in _orders:
        _orders[nx, rows, po] = tree.local_index(nx, rows, *frame_cases.pixel_order(po, False, nx, rows))
    return scene.camera, prm, rt.accum_frame_id(scene.camera, prm), _orders[nx, rows, po]


def _state_of(rt, st):
    return rt.AccumState(st["nx"], st["rows"], st["first_sample"], st["done"], st["planes"], st["frame_id"], sum=st["sum"], moments=st["moments"],
                         counts=st["counts"], converged=st["converged"], channel_moments=st["channel_moments"])


def _import(rt, r, cam, prm, fid, st):
    st["frame_id"] = fid
    s = _state_of(rt, st)
    r.accum_begin(cam, prm)
    r.accum_import(s)
    return s


def _exports_what_was_imported(r, s, what):
    e = r.accum_export()
    for k in ("nx", "rows", "first_sample", "done", "planes", "frame_id"):
        assert getattr(e, k) == getattr(s, k), (what, k)
    for name in ("sum", "moments", "channel_moments") + (("counts", "converged") if s.adaptive else ()):
        a, b = getattr(e, name), getattr(s, name)
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            _same(a, b, (what, "export", name))


def _tree_figures(st, loc):
    ybar, v = ds.figures(st)
    return tree.figures(tree.to_local(ybar, loc), tree.to_local(v, loc), int(ds.pixel_counts(st).min()))


def _read_out_is_the_reference(rt, r, st, loc, what):
    """accum_read, the export, the counts and — from two samples on — both filters of the open accumulation against the references on `st`."""
    w = st["where"]
    adaptive, channels = bool(st["planes"] & ref.COUNTS), bool(st["planes"] & ref.CHANNELS)
    cnt = ds.pixel_counts(st)
    img, rgb8, sem, noise = r.accum_read(want_rgb8=True, want_sem=True)
    want_img = ds.image(st)
    _held(img, want_img, (what, "f32"), w)
    _held(rgb8, denoise_ref.finalize_rgb8(want_img), (what, "rgb8"), {k: m[::-1] for k, m in w.items()})
    ybar, v = ds.figures(st)
    with np.errstate(all="ignore"):
        _held(sem, np.sqrt(v).astype(np.float32), (what, "sem"), w)
    _figures_are(noise, _tree_figures(st, loc), int(cnt.max()), what)
    counts, info = r.accum_counts()
    assert np.array_equal(counts, cnt), (what, "counts")
    conv = st["converged"] if adaptive else np.zeros_like(cnt, np.uint8)
    want_info = tree.adaptive_info(tree.to_local(cnt, loc), tree.to_local(conv, loc))
    rp = adaptive_ref.Replay([np.zeros(st["sum"].shape, np.float32)])
    rp.cnt, rp.conv = cnt, conv.astype(bool)
    assert (info.n_active, info.n_samples, info.spp_min, info.spp_max) == want_info == rp.info(), (what, "info")
    if channels:
        s1c, s2c = ds.channel_planes(st)
        with np.errstate(all="ignore"):
            want_sem = denoise_channels_ref.channel_sem(s1c, s2c, cnt)
        _held(r.accum_channel_sem(), want_sem, (what, "channel sem"), w)
    if st["done"] < 2:
        return
    strength = rt._ffi.DENOISE_DEFAULT_STRENGTH
    c, y, vf = ds.denoise_inputs(st)
    clean = np.isfinite(c).all(axis=-1)
    got = r.accum_denoise()[0]
    _held(got, denoise_ref.denoise(c, y, vf, 5, 1, strength)[0], (what, "the filter"), w)
    assert np.isfinite(got[clean]).all() and (~clean).sum() == 9, (what, "a non-finite pixel spread", int((~np.isfinite(got[clean])).sum()))
    _held(got[~clean], c[~clean], (what, "a non-finite pixel stays what it is"))
    if channels:
        c, var = ds.channel_inputs(st)
        got = r.accum_denoise_channels()[0]
        _held(got, denoise_channels_ref.denoise(c, var, 5, 1, strength)[0], (what, "the colour-guided filter"), w)
        assert np.isfinite(got[clean]).all(), (what, "a non-finite pixel spread through the colour-guided filter")
        _held(got[~clean], c[~clean], (what, "a non-finite pixel stays what it is, colour-guided"))


def _finite_figures_are_the_tree(rt, r, cam, prm, fid, st, loc, what):
    """The state with its non-finite luminance figures replaced (designed_states.finite_copy) — once keeping every finite magnitude, once
    with the moments within 1e10, where every addition of the tree rounds — imported and read: mean_luminance, rms_sem and noise are
    numbers, held to the tree bit for bit and to math.fsum within noise_tree_ref.figure_bound.  With nb <= 4 partial sums the longest chain
    is d = 9 + 1 + 9 = 19 additions; mean_luminance, whose terms have both signs (the class "negative s1"), is bounded relative to
    (sum |Ybar|) / npix, rms_sem — its terms are clamped at 0 — relative to itself."""
    for limit in (None, 1e10):
        fin = ds.finite_copy(st, limit)
        _import(rt, r, cam, prm, fid, fin)
        noise = r.accum_read()[3]
        ybar, v = ds.figures(fin)
        cnt = ds.pixel_counts(fin)
        want = tree.figures(tree.to_local(ybar, loc), tree.to_local(v, loc), int(cnt.min()))
        assert np.isfinite(want[:2]).all() and (np.isfinite(want[2]) or cnt.min() < 2), (what, limit, want)
        _figures_are(noise, want, int(cnt.max()), (what, "finite figures", limit))
        mean, rms, _ = tree.exact_figures(ybar, v)
        bound = tree.figure_bound(ybar.size)[0]
        assert abs(noise.mean_luminance - mean) <= bound * tree.abs_mean(ybar), (what, limit, noise.mean_luminance, mean)
        assert abs(noise.rms_sem - rms) <= bound * rms, (what, limit, noise.rms_sem, rms)


# ---- 1. a uniform state: the <false> forms of k_finalize, k_sem, k_noise_partials, k_noise_final, k_denoise_inputs, k_channel_sem, ... ----
@pytest.mark.parametrize("channels", [False, True])
@pytest.mark.parametrize("done", ds.UNIFORM_DONE)
@pytest.mark.parametrize("nx,rows", SMALL_FRAMES)
def test_read_out_of_a_uniform_state(rt, ctx, nx, rows, done, channels):
    cam, prm, fid, loc = _begin(rt, ctx, nx, rows)
    st = ds.state(nx, rows, done, channels=channels)
    s = _import(rt, ctx, cam, prm, fid, st)
    what = (nx, rows, done, "channels" if channels else "")
    _read_out_is_the_reference(rt, ctx, st, loc, what)
    _exports_what_was_imported(ctx, s, what)
    _finite_figures_are_the_tree(rt, ctx, cam, prm, fid, st, loc, what)
    ctx.accum_end()


# ---- 2. the same with counts: the <true> forms of k_finalize, k_sem, k_noise_*, k_denoise_inputs, and k_adaptive_decide<false> ------------
@pytest.mark.parametrize("channels", [False, True])
@pytest.mark.parametrize("done", ds.COUNTS_DONE)
@pytest.mark.parametrize("nx,rows", SMALL_FRAMES)
def test_read_out_of_a_state_with_counts(rt, ctx, nx, rows, done, channels):
    cam, prm, fid, loc = _begin(rt, ctx, nx, rows)
    st = ds.state(nx, rows, done, counts=True, channels=channels)
    s = _import(rt, ctx, cam, prm, fid, st)
    what = (nx, rows, done, "counts", "channels" if channels else "")
    if done == 4294967295:
        assert int(st["counts"].astype(np.uint64).sum()) > 2 ** 32 and ((st["counts"] > 2 ** 31) & (st["converged"] == 1)).any()
    _read_out_is_the_reference(rt, ctx, st, loc, what)
    _exports_what_was_imported(ctx, s, what)
    _finite_figures_are_the_tree(rt, ctx, cam, prm, fid, st, loc, what)
    ctx.accum_end()


@pytest.mark.parametrize("nx,rows", SMALL_FRAMES)
@pytest.mark.parametrize("done", [0, 1, 2])
def test_noise_is_inf_exactly_when_a_pixel_holds_fewer_than_two_samples(rt, ctx, nx, rows, done):
    """An adaptive state of 0 and of 1 issued samples, every pixel active, its figures numbers (designed_states.finite_copy): the read-out
    divides by 1, mean_luminance is the tree's, rms_sem is 0 and the noise is +inf; at 2 samples the noise is a number."""
    cam, prm, fid, loc = _begin(rt, ctx, nx, rows)
    st = ds.finite_copy(ds.state(nx, rows, done, counts=True), 1e10)
    s = _import(rt, ctx, cam, prm, fid, st)
    img, _, sem, noise = ctx.accum_read(want_sem=True)
    _held(img, (st["sum"] / np.float32(max(done, 1))).astype(np.float32), (done, "the read-out divides by max(n, 1)"), st["where"])
    want = _tree_figures(st, loc)
    assert np.isfinite(want[:2]).all() and (want[0] > 0) == (done > 0)
    _figures_are(noise, want, done, (nx, rows, "adaptive, done", done))
    assert (noise.noise == np.inf) == (done < 2) and (done < 2 or (np.isfinite(noise.noise) and noise.noise > 0))
    if done < 2:
        assert not sem.any() and noise.rms_sem == 0.0
    _exports_what_was_imported(ctx, s, done)
    ctx.accum_end()


# ---- 3. more than 256 partial sums: the second trip of k_noise_final<false>, k_noise_final<true> and k_adaptive_info -----------------------
@pytest.mark.parametrize("po", [1, 2])
@pytest.mark.parametrize("nx,rows", BIG_FRAMES)
def test_more_than_256_partial_sums(rt, ctx, nx, rows, po):
    """The frame's extremes lie in pixels whose local index is above 65536 (designed_states.big_state), so a final loop that stops after
    its first trip changes every figure and n_active, spp_min and spp_max.

    The bound against math.fsum (noise_tree_ref.figure_bound): a term passes through at most d = 9 + ceil(nb / 256) + 9 additions — 6
    lane steps and 3 wave steps in its workgroup, one per trip of the final loop, 6 + 3 again; nb = 257 or 258, so d = 20.  Sums of
    non-negative terms: relative error at most (1 + 2^-53)^d - 1.  The division by npix adds one rounding, the square root halves the
    error and adds one; the exact figures themselves carry two.  Hence (d + 4) 2^-53 = 24 * 2^-53 for mean_luminance and rms_sem, and
    twice that plus one rounding for their quotient."""
    cam, prm, fid, loc = _begin(rt, ctx, nx, rows, po)
    tiled = frame_cases.pixel_order(po, False, nx, rows)[0] > 0
    assert tiled == (po == 2 and nx % 8 == 0) and (loc.reshape(-1) != np.arange(nx * rows)).any() == tiled
    assert tree.chain_length(nx * rows) == 20
    for kind in ("uniform", "counts", "nan"):
        st = ds.big_state(nx, rows, loc, kind)
        _import(rt, ctx, cam, prm, fid, st)
        what = (nx, rows, po, kind)
        noise = ctx.accum_read()[3]
        want = _tree_figures(st, loc)
        _figures_are(noise, want, int(ds.pixel_counts(st).max()), what)
        ybar, v = ds.figures(st)
        cut = tree.figures(tree.to_local(ybar, loc), tree.to_local(v, loc), 2, tail=False)
        assert [_figure_bits(x) for x in cut] != [_figure_bits(x) for x in want]
        if kind != "nan":
            for got, exact, bound in zip((noise.mean_luminance, noise.rms_sem, noise.noise), tree.exact_figures(ybar, v), tree.figure_bound(nx * rows)):
                print(f"{what}: {got!r} against the exact {exact!r}: {abs(got - exact) / exact:.3e}, bound {bound:.3e}")
                assert abs(got - exact) <= bound * exact, (what, got, exact, bound)
        counts, info = ctx.accum_counts()
        assert np.array_equal(counts, ds.pixel_counts(st)), what
        got = (info.n_active, info.n_samples, info.spp_min, info.spp_max)
        if kind == "counts":
            cl, fl = tree.to_local(st["counts"], loc), tree.to_local(st["converged"], loc)
            assert got == tree.adaptive_info(cl, fl) == (1, int(st["counts"].astype(np.uint64).sum()), 2, 2 ** 32 - 1), (what, got)
            assert got != tree.adaptive_info(cl, fl, tail=False) and info.n_samples > 2 ** 32
        else:  # a uniform accumulation: every pixel active with `done` samples
            assert got == (nx * rows, nx * rows * 24, 24, 24) == tree.adaptive_info(np.full(nx * rows, 24), np.zeros(nx * rows)), (what, got)
    ctx.accum_end()


@pytest.mark.parametrize("nx,rows", SMALL_FRAMES)
def test_the_order_of_the_waves_is_part_of_the_figures(rt, ctx, nx, rows):
    """((w0 + w1) + w2) + w3 on terms for which the same sum with w2 and w3 exchanged rounds to another value (designed_states.WAVE_TERMS)."""
    cam, prm, fid, loc = _begin(rt, ctx, nx, rows)
    st = ds.wave_order_state(nx, rows, loc)
    _import(rt, ctx, cam, prm, fid, st)
    noise = ctx.accum_read()[3]
    want = _tree_figures(st, loc)
    assert want[:2] == (ds.WAVE_SUM / (nx * rows), float(np.sqrt(ds.WAVE_SUM / (nx * rows)))) and ds.WAVE_SUM != ds.WAVE_SUM_SWAPPED
    _figures_are(noise, want, 2, (nx, rows, "wave order"))
    ctx.accum_end()


# ---- 4. the decision: k_adaptive_decide<true> on the thresholds ---------------------------------------------------------------------------
@pytest.mark.parametrize("tolerance,min_samples", [(TOLERANCE, 8), (TOLERANCE, 9), (0.0, 8)])
def test_the_decision_on_the_thresholds(rt, ctx, tolerance, min_samples):
    nx, rows, n = 24, 16, 8
    cam, prm, fid, _ = _begin(rt, ctx, nx, rows)
    st = ds.threshold_state(nx, rows, n, TOLERANCE, FLOOR)
    _import(rt, ctx, cam, prm, fid, st)
    stats = ctx.accum_add_adaptive(1, tolerance, FLOOR, min_samples)
    e = ctx.accum_export()
    s1, s2, w = st["moments"][..., 0], st["moments"][..., 1], st["where"]
    was = st["converged"] == 1
    want = was | adaptive_ref.converged(s1, s2, n, tolerance, FLOOR, min_samples)
    got = e.converged == 1
    wrong = sorted(k for k, m in w.items() if (m & (got != want)).any())
    assert np.array_equal(got, want), ("the decision differs from adaptive_ref.converged in the classes", wrong, int((got != want).sum()))
    assert got[was].all(), "a pixel imported as converged was looked at again"
    assert e.done == n + 1 and stats.n_paths == int((~want).sum())
    assert (e.counts[~want] == n + 1).all() and np.array_equal(e.counts[want], st["counts"][want])
    _same(e.sum[want], st["sum"][want], "the sums of the converged pixels")
    _same(e.moments[want], st["moments"][want], "the moments of the converged pixels")
    if (tolerance, min_samples) == (TOLERANCE, 8):  # both decisions in every pair of classes
        for stem in ("straddle", "ybar floor", "ybar above floor", "ybar below floor", "negative ybar"):
            assert got[w[stem + " le"]].all() and not got[w[stem + " gt"]].any(), stem
        assert got[w["v exact"]].all() and got[w["v pred"]].all() and not got[w["v succ"]].any() and not got[w["nan v"]].any()
    elif min_samples == 9:
        assert np.array_equal(got, was)
    else:
        assert got[w["v zero"]].all() and not got[w["v exact"]].any() and 0 < (got & ~was).sum() < 16
    ctx.accum_end()


# ---- 5. a pixel that stopped on fewer than two samples ------------------------------------------------------------------------------------
def test_a_pixel_that_stopped_on_fewer_than_two_samples_spreads_to_no_other(rt, ctx):
    """rt_accum_state_check accepts a converged pixel with counts 0 or 1 beside done = 8.  The header: rt_accum_read divides it by
    max(n_p, 1); rt_accum_denoise gives it that colour and a NaN guide, so it stays what it is and every other pixel stays finite.
    (k_denoise_inputs<true> once formed sum / (float)0 beside the finite guide (0, 0): in this neighbourhood the reference with those
    inputs returns inf in the 121 pixels of the search window — tests/test_designed_states_host.py.)"""
    nx, rows = SMALL_FRAMES[0]
    cam, prm, fid, loc = _begin(rt, ctx, nx, rows)
    st = ds.stopped_early_state(nx, rows)
    w = st["where"]
    few = w["count 0"] | w["count 1"]
    s = _import(rt, ctx, cam, prm, fid, st)
    assert s.check() and ref.state_check(st)
    img, _, sem, noise = ctx.accum_read(want_sem=True)
    _held(img, ds.image(st), "f32", w)
    _same(img[few], st["sum"][few], "a pixel with 0 or 1 samples is its sum / 1")
    assert not sem[few].any() and np.isfinite(sem).all() and noise.noise == np.inf and noise.spp_done == 8
    strength = rt._ffi.DENOISE_DEFAULT_STRENGTH
    c, y, v = ds.denoise_inputs(st)
    assert np.isnan(y[few]).all() and np.isnan(v[few]).all() and np.isfinite(c).all()
    got = ctx.accum_denoise()[0]
    _held(got, denoise_ref.denoise(c, y, v, 5, 1, strength)[0], "the filter", w)
    assert np.isfinite(got).all(), ("non-finite pixels", int((~np.isfinite(got).all(axis=-1)).sum()))
    _same(got[few], img[few], "the two pixels stay what rt_accum_read returns")
    assert (_bits(got[~few]) != _bits(img[~few])).mean() > 0.9  # (the filter did filter the others)
    cc, var = ds.channel_inputs(st)
    got = ctx.accum_denoise_channels()[0]
    _held(got, denoise_channels_ref.denoise(cc, var, 5, 1, strength)[0], "the colour-guided filter", w)
    assert np.isfinite(got[~w["count 0"]]).all(), "a pixel without a sample spread through the colour-guided filter"
    _exports_what_was_imported(ctx, s, "stopped early")
    ctx.accum_end()


# ---- 6. a uniform accumulation behind an adaptive one on the same context -----------------------------------------------------------------
def _every_read_out(r):
    """Every read-out of the open accumulation (channels and halves tracked, done >= 4), by name; arrays, and ctypes figures as their bytes."""
    out = {}
    out["read f32"], out["read rgb8"], out["read sem"], noise = r.accum_read(want_rgb8=True, want_sem=True)
    out["counts"], info = r.accum_counts()
    out["denoise f32"], out["denoise rgb8"] = r.accum_denoise(want_rgb8=True)
    out["channel sem"] = r.accum_channel_sem()
    out["denoise channels f32"], out["denoise channels rgb8"] = r.accum_denoise_channels(want_rgb8=True)
    for h in (0, 1):
        out[f"half {h} f32"], out[f"half {h} sem"] = r.accum_half(h, want_sem=True)
    out["denoise halves f32"], out["denoise halves rgb8"], out["denoise halves err"], res = r.accum_denoise_halves(want_rgb8=True, want_err=True)
    e = r.accum_export()
    for name in ("sum", "moments", "counts", "converged", "channel_moments"):
        out["export " + name] = getattr(e, name)
    out["export scalars"] = np.array([e.nx, e.rows, e.first_sample, e.done, e.planes, e.frame_id], np.uint64)
    for name, figures in (("noise", noise), ("info", info), ("residual", res)):
        out[name] = np.frombuffer(bytes(figures), np.uint8)
    return out


def test_a_uniform_accumulation_never_reads_a_stale_count_plane(rt, ctx):
    """The readers of a uniform accumulation are handed the context's count plane whatever it holds (K<false> does not read it).  Here it
    holds the n_p of an ended adaptive accumulation of the same size, which differ from pixel to pixel; a fresh context has none at all.
    Every read-out of the two is the same, byte for byte."""
    nx, rows = SMALL_FRAMES[0]
    cam, prm, fid, _ = _begin(rt, ctx, nx, rows)
    st = ds.state(nx, rows, 24, counts=True, channels=True)
    assert len(np.unique(st["counts"])) > 2
    _import(rt, ctx, cam, prm, fid, st)
    assert np.array_equal(ctx.accum_counts()[0], st["counts"])
    ctx.accum_end()
    fresh = rt.Renderer(0)
    try:
        fresh.upload(_scenes[nx, rows])
        outs = []
        for r in (ctx, fresh):
            r.accum_begin(cam, prm)
            r.accum_track_channels()
            r.accum_track_halves()
            r.accum_add(3)
            r.accum_add(2)
            outs.append(_every_read_out(r))
            r.accum_end()
    finally:
        fresh.close()
    stale, clean = outs
    assert stale["export scalars"][3] == 5 and (stale["counts"] == 5).all() and not stale["export converged"].any()
    assert stale.keys() == clean.keys()
    for name in stale:
        _same(stale[name], clean[name], name)
