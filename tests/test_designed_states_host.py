"""tests/designed_states.py and tests/noise_tree_ref.py on the references alone (no GPU): every designed state has the property it is built
for — else tests/test_designed_states.py would hold the kernels to states that cannot tell a right kernel from a wrong one.  The measured
shares are printed."""
import math

import numpy as np
import pytest

import adaptive_ref
import designed_states as ds
import frame_cases
import noise_ref
import noise_tree_ref as tree

SMALL_FRAMES = ((40, 20), (37, 21))
BIG_FRAMES = ((257, 256), (264, 250))


def test_every_quantisation_step_is_reached_from_both_sides():
    b = ds.quantisation_boundaries()
    assert b.size == 255 and len(set(b.tolist())) == 255 and (b[0], b[-1]) == (0x37800290, 0x3F7E0612), (hex(b[0]), hex(b[-1]))
    k = np.arange(1, 256)
    assert np.array_equal(ds.quantise(ds.f32_of_bits(b)), k) and np.array_equal(ds.quantise(ds.f32_of_bits(b - 1)), k - 1)
    # the special values: +0, -0, the denormal, FLT_MIN, 1 - ulp, 1, 1 + ulp, FLT_MAX, +inf, -inf, -1, NaN
    assert ds.quantise(ds.f32_of_bits(ds.SPECIAL_BITS)).tolist() == [0, 0, 0, 0, 255, 255, 255, 255, 255, 0, 0, 0]
    for nx, rows in SMALL_FRAMES:  # in the state: every step from both sides in every channel, the channels of a pixel on different steps
        st = ds.state(nx, rows, 1)
        q = ds.quantise(ds.image(st).reshape(-1)).reshape(rows, nx, 3)[st["where"]["quant"]].astype(int)
        raw = st["sum"][st["where"]["quant"]].view(np.uint32)
        for ch in range(3):
            for side, want in ((b, k), (b - 1, k - 1)):
                at = np.searchsorted(np.sort(raw[:, ch]), side)
                assert np.array_equal(np.sort(raw[:, ch])[at], side)
                assert np.array_equal(q[:, ch][np.argsort(raw[:, ch])][at], want), (nx, rows, ch)
        on_a_step = q[:len(b) * 2]
        assert ((on_a_step[:, 0] != on_a_step[:, 1]) & (on_a_step[:, 1] != on_a_step[:, 2])).mean() > 0.98


def test_float_of_a_large_count_rounds():
    assert np.float32(16777217) == 16777216 and float(np.float32(4294967295)) == 2.0 ** 32
    for nx, rows in SMALL_FRAMES:
        for done in ds.LARGE_DONE:
            for counts in (False, True):
                st = ds.state(nx, rows, done, counts=counts)
                a, b = ds.image(st), ds.image_f64(st)
                differ = int((a.view(np.uint32) != b.view(np.uint32)).sum())
                print(f"{nx} x {rows}, done {done}, counts {counts}: the f32 and the f64 quotient differ in {differ} of {a.size} values")
                assert differ >= 1
                if counts:  # the counts of the converged pixels pass 2^31, the samples of the frame 2^32
                    cnt = st["counts"]
                    assert (cnt[st["converged"] == 1] >= 2).all() and (cnt[st["converged"] == 0] == done).all()
                    assert int(cnt.astype(np.uint64).sum()) > 2 ** 32 and (done < 2 ** 31 or ((cnt > 2 ** 31) & (st["converged"] == 1)).any())


@pytest.mark.parametrize("n", [3, 7, 24, 64, 1000, 16777217, 4294967295])
def test_constant_samples_cancel_to_both_sides_of_zero(n):
    """The shares are taken over the blocks at the magnitudes 1e-30, 1 and 1e30 together.  The blocks at 1e-160 and 1e150 are left out of
    them: at 1e-160 y y is a denormal of a few bits (every S2 is a multiple of 2^-1074 and q is mostly negative), at 1e150 S1 S1 overflows
    from n of some 10^7 on (q is NaN); both stay in the state as what they are, very small and very large moments."""
    for nx, rows in SMALL_FRAMES:
        st = ds.state(nx, rows, n)
        q = ds.variance_before_clamp(st["moments"][..., 0], st["moments"][..., 1], n)
        pooled = np.zeros_like(st["where"]["zero"])
        for mag in ds.NORMAL_MAGNITUDES:  # (the shares do not depend on the magnitude: pooled, so that the sample is a few hundred pixels)
            m = st["where"]["const %g" % mag]
            pooled |= m
            print(f"{nx} x {rows}, n {n}, magnitude {mag:g}: q < 0 in {float((q[m] < 0).mean()):.2f}, q > 0 in {float((q[m] > 0).mean()):.2f} of {int(m.sum())} pixels")
        neg, pos = float((q[pooled] < 0).mean()), float((q[pooled] > 0).mean())
        print(f"{nx} x {rows}, n {n}, the constant-sample blocks: q < 0 in {neg:.2f}, q > 0 in {pos:.2f} of {int(pooled.sum())} pixels")
        assert neg >= 0.25 and pos >= 0.25, (n, neg, pos)
        for name in ("s2 zero", "negative s1"):  # a negative q of full size, and a plain variance under a negative mean
            assert ((q[st["where"][name]] < 0) == (name == "s2 zero")).all()
        ybar, v = ds.figures(st)
        assert (v[st["where"]["s2 zero"]] == 0).all() and (ybar[st["where"]["negative s1"]] < 0).all() and np.isnan(v[st["where"]["non-finite"]]).any()
        assert np.isinf(v[st["where"]["non-finite"]]).any()  # (S1 = inf alone gives q = -inf: the clamp's 0)
        assert np.isnan(v[st["where"]["non_finite_sum"]]).all() and st["where"]["non_finite_sum"].sum() == 9


def test_two_constant_samples_leave_no_variance():
    st = ds.state(40, 20, 2)
    q = ds.variance_before_clamp(st["moments"][..., 0], st["moments"][..., 1], 2)
    for mag in ds.NORMAL_MAGNITUDES:
        assert (q[st["where"]["const %g" % mag]] == 0).all()


def test_channel_classes_are_independent_between_channels():
    st = ds.state(40, 20, 7, channels=True)
    w = st["where"]
    for a in range(3):
        for b in range(a + 1, 3):
            assert not (w["ch%d non-finite" % a] & w["ch%d non-finite" % b]).any()
    s1, s2 = ds.channel_planes(st)
    q = ds.variance_before_clamp(s1, s2, 7)
    for ch in range(3):
        m = w["ch%d const 1" % ch]
        assert (q[..., ch][m] < 0).mean() >= 0.25 and (q[..., ch][m] > 0).mean() >= 0.25


def test_threshold_blocks_hold_both_decisions():
    tol, floor, n = 0.05, 0.01, 8
    st = ds.threshold_state(24, 16, n, tol, floor)
    s1, s2, w = st["moments"][..., 0], st["moments"][..., 1], st["where"]
    assert set(w) == set(ds.THRESHOLD_CLASSES)
    v, t = noise_ref.pixel_figures(s1, s2, n)[1], ds.threshold_of(s1, n, tol, floor)
    conv = adaptive_ref.converged(s1, s2, n, tol, floor, 8)
    active = st["converged"] == 0
    for name, eq in (("v exact", t), ("floor branch exact", t), ("v succ", np.nextafter(t, np.inf)), ("floor branch succ", np.nextafter(t, np.inf)),
                     ("v pred", np.nextafter(t, -np.inf)), ("floor branch pred", np.nextafter(t, -np.inf))):
        assert w[name].any() and (v[w[name]] == eq[w[name]]).all(), name
        assert (conv[w[name]] == (not name.endswith("succ"))).all(), name
    for stem in ("straddle", "ybar floor", "ybar above floor", "ybar below floor", "negative ybar"):
        assert conv[w[stem + " le"]].all() and not conv[w[stem + " gt"]].any(), stem
    ybar = s1 / n
    assert (ybar[w["ybar floor le"]] == floor).all() and (ybar[w["ybar above floor le"]] == np.nextafter(floor, 1)).all()
    assert (ybar[w["ybar below floor le"]] == np.nextafter(floor, 0)).all() and (ybar[w["negative ybar le"]] < 0).all()
    assert t[w["ybar above floor le"]][0] > t[w["ybar floor le"]][0] == t[w["ybar below floor le"]][0]  # one ulp of Ybar moves the threshold
    assert not np.isfinite(v[w["nan v"]]).any() and np.isnan(v[w["nan v"]]).sum() == 3 and not conv[w["nan v"]].any() and (v[w["v zero"]] == 0).all() and conv[w["v zero"]].all()
    assert not conv[w["imported converged"]].any() and not active[w["imported converged"]].any() and active[~w["imported converged"]].all()
    share = float(conv[active].mean())
    zero = adaptive_ref.converged(s1, s2, n, 0.0, floor, 8)
    print(f"threshold state: {int(w['v exact'].sum())} / {int(w['v succ'].sum())} / {int(w['v pred'].sum())} pixels exactly on, above and below the "
          f"threshold; {share:.2f} of the active pixels converge at tolerance {tol}, {int(zero[active].sum())} at tolerance 0")
    assert 0.25 <= share <= 0.75 and 0 < zero[active].sum() < 16 and np.array_equal(zero[active], (v[active] == 0))
    assert not adaptive_ref.converged(s1, s2, n, tol, floor, 9).any()


def test_tree_reference_against_plain_sums():
    rng = np.random.default_rng(9)
    one = np.array([0.3])
    assert tree.tree_sum(one) == 0.0 + 0.3 and tree.figures(one, np.array([0.04]), 2) == (0.3, 0.2, 0.2 / 0.3)
    assert tree.figures(one, one, 1)[2] == np.inf and tree.figures(np.zeros(3), np.zeros(3), 2)[2] == 0.0
    assert tree.figures(np.zeros(3), np.ones(3), 2)[2] == np.inf and np.isnan(tree.figures(np.array([np.nan, 1.0]), np.ones(2), 2)[2])
    for npix in (1, 63, 64, 255, 256, 257, 800, 65536, 65792):
        x = rng.uniform(0.0, 1.0, npix) * 10.0 ** rng.uniform(-6, 6, npix)
        got, exact = tree.tree_sum(x), math.fsum(x)
        bound = tree.chain_length(npix) * tree.U
        print(f"{npix} terms: tree / exact - 1 = {got / exact - 1:.3e}, np.sum / exact - 1 = {float(np.sum(x)) / exact - 1:.3e}, bound {bound:.3e}")
        assert abs(got - exact) <= bound * exact and abs(got - float(np.sum(x))) <= (bound + npix * tree.U) * exact
    # the order matters: the tree is neither the sequential sum nor numpy's pairwise sum on a frame of a few hundred pixels
    x = rng.uniform(0.0, 1.0, 800)
    seq = 0.0
    for t in x:
        seq += t
    assert tree.tree_sum(x) != seq or tree.tree_sum(x[::-1].copy()) != tree.tree_sum(x)
    # the integer sums: plain sums, minima and maxima; 64-bit, nothing wraps at 2^32
    cnt = rng.integers(2, 2 ** 32, 70000).astype(np.uint32)
    conv = (rng.random(70000) < 0.5).astype(np.uint8)
    assert tree.adaptive_info(cnt, conv) == (int((conv == 0).sum()), int(cnt.astype(np.uint64).sum()), int(cnt.min()), int(cnt.max()))
    assert tree.adaptive_info(cnt, conv)[1] > 2 ** 32


@pytest.mark.parametrize("nx,rows", BIG_FRAMES)
@pytest.mark.parametrize("po", [1, 2])
def test_big_frames_reach_the_tail_of_the_final_loop(nx, rows, po):
    tpr, tp = frame_cases.pixel_order(po, False, nx, rows)
    assert (tpr > 0) == (po == 2 and nx % 8 == 0)
    loc = tree.local_index(nx, rows, tpr, tp)
    assert np.array_equal(np.sort(loc.reshape(-1)), np.arange(nx * rows)) and -(-nx * rows // 256) > 256
    for kind in ("uniform", "counts", "nan"):
        st = ds.big_state(nx, rows, loc, kind)
        ybar, v = ds.figures(st)
        yl, vl = tree.to_local(ybar, loc), tree.to_local(v, loc)
        spp_min = int(ds.pixel_counts(st).min())
        whole, cut = tree.figures(yl, vl, spp_min), tree.figures(yl, vl, spp_min, tail=False)
        print(f"{nx} x {rows}, order {po}, {kind}: figures {whole}, without the second trip {cut}")
        if kind == "nan":
            assert all(np.isnan(x) for x in whole) and not any(np.isnan(x) for x in cut)
            continue
        assert cut[0] < 0.95 * whole[0] and cut[1] < 0.2 * whole[1]  # the bright pixel and the largest V lie in the tail
        for a, b, bound in zip(whole, tree.exact_figures(ybar, v), tree.figure_bound(nx * rows)):
            assert abs(a - b) <= bound * b, (kind, a, b, bound)
        if kind == "counts":
            cl, fl = tree.to_local(st["counts"], loc), tree.to_local(st["converged"], loc)
            info, info_cut = tree.adaptive_info(cl, fl), tree.adaptive_info(cl, fl, tail=False)
            assert info == (1, int(st["counts"].astype(np.uint64).sum()), 2, 2 ** 32 - 1) and info[1] > 2 ** 32
            assert info_cut[0] == 0 and info_cut[2] > 2 and info_cut[3] <= 2 ** 31 and info_cut[1] < info[1]


@pytest.mark.parametrize("done,counts", [(7, False), (24, True), (4294967295, True)])
def test_in_the_references_a_non_finite_pixel_spreads_to_no_other(done, counts):
    """What the GPU test asserts of both filters holds of both references on the designed states: the nine pixels with a non-finite sum
    come back as they are, and every other pixel comes back finite."""
    import denoise_channels_ref
    import denoise_ref
    st = ds.state(40, 20, done, counts=counts, channels=True)
    c, y, v = ds.denoise_inputs(st)
    clean = np.isfinite(c).all(axis=-1)
    assert (~clean).sum() == 9 and np.array_equal(~clean, st["where"]["non_finite_sum"])
    out = denoise_ref.denoise(c, y, v, 5, 1, 1.0)[0]
    assert np.isfinite(out[clean]).all() and np.array_equal(out[~clean].view(np.uint32), c[~clean].view(np.uint32))
    s1c, s2c = ds.channel_planes(st)
    with np.errstate(all="ignore"):
        var = denoise_channels_ref.channel_variance(s1c, s2c, ds.pixel_counts(st)).astype(np.float32)
    out = denoise_channels_ref.denoise(c, var, 5, 1, 1.0)[0]
    assert np.isfinite(out[clean]).all() and np.array_equal(out[~clean].view(np.uint32), c[~clean].view(np.uint32))


def test_the_wave_order_state_tells_the_order_of_the_waves():
    a, b, c = ds.WAVE_TERMS
    assert (a + b) + c == ds.WAVE_SUM and (a + c) + b == ds.WAVE_SUM_SWAPPED and ds.WAVE_SUM != ds.WAVE_SUM_SWAPPED
    for (nx, rows), po in ((SMALL_FRAMES[0], 2), (SMALL_FRAMES[1], 1)):
        loc = tree.local_index(nx, rows, *frame_cases.pixel_order(po, False, nx, rows))
        st = ds.wave_order_state(nx, rows, loc)
        ybar, v = ds.figures(st)
        yl, vl = tree.to_local(ybar, loc), tree.to_local(v, loc)
        assert (yl[0], yl[128], yl[192]) == ds.WAVE_TERMS == (vl[1], vl[129], vl[193]) and np.count_nonzero(yl) == 3 == np.count_nonzero(vl)
        assert tree.tree_sum(yl) == ds.WAVE_SUM == tree.tree_sum(vl)
        assert tree.figures(yl, vl, 2)[0] == ds.WAVE_SUM / (nx * rows)


@pytest.mark.parametrize("counts", [False, True])
@pytest.mark.parametrize("nx,rows", SMALL_FRAMES)
def test_the_finite_copies_have_figures_that_are_numbers(nx, rows, counts):
    """ds.state holds NaN moments, so its frame figures are NaN; finite_copy is the state on which the figures are held to the tree.  Its
    figures are finite for every `done`, positive, and — moments within 1e10 — differ under another order of the waves."""
    loc = tree.local_index(nx, rows, *frame_cases.pixel_order(0, False, nx, rows))
    for done in (ds.COUNTS_DONE if counts else ds.UNIFORM_DONE) + (0,):
        raw = ds.state(nx, rows, done, counts=counts)
        if done >= 1:
            assert np.isnan(tree.figures(*(tree.to_local(a, loc) for a in ds.figures(raw)), done)[0])
        for limit in (None, 1e10):
            st = ds.finite_copy(raw, limit)
            ybar, v = ds.figures(st)
            assert np.isfinite(ybar).all() and np.isfinite(v).all() and (v >= 0).all() and 0 < st["where"]["replaced"].sum() < 0.4 * nx * rows
            mean, rms, noise = tree.figures(tree.to_local(ybar, loc), tree.to_local(v, loc), int(ds.pixel_counts(st).min()))
            print(f"{nx} x {rows}, done {done}, counts {counts}, limit {limit}: {mean!r}, {rms!r}, {noise!r}; {int(st['where']['replaced'].sum())} pixels replaced")
            assert np.isfinite(mean) and np.isfinite(rms) and (mean > 0) == (done > 0) and (rms > 0) == (done >= 2) and (np.isfinite(noise) == (done >= 2))
            assert (ybar < 0).any() == (done > 0)  # the class "negative s1" stays
            exact = tree.exact_figures(ybar, v)
            bound = tree.figure_bound(nx * rows)[0]
            assert abs(mean - exact[0]) <= bound * tree.abs_mean(ybar) and abs(rms - exact[1]) <= bound * exact[1]


def test_the_stopped_early_state_tells_a_finite_guide_from_a_nan_guide():
    """With the inputs k_denoise_inputs<true> once formed — c = sum / (float)n_p, the guide of pixel_noise — the reference filter returns
    a non-finite colour in the whole search window of the pixel without a sample; with the header's inputs every pixel is finite."""
    import denoise_ref
    st = ds.stopped_early_state(40, 20)
    w = st["where"]
    assert w["count 0"].sum() == 1 == w["count 1"].sum() and st["converged"][w["count 0"] | w["count 1"]].all()
    c, y, v = ds.denoise_inputs(st)
    out = denoise_ref.denoise(c, y, v, 5, 1, 1.0)[0]
    assert np.isfinite(out).all()
    ybar, var = ds.figures(st)
    with np.errstate(all="ignore"):
        c_old = (st["sum"] / ds.pixel_counts(st).astype(np.float32)[..., None]).astype(np.float32)
    assert np.isinf(c_old[w["count 0"]]).all() and (ybar[w["count 0"]] == 0).all() and (var[w["count 0"] | w["count 1"]] == 0).all()
    old = denoise_ref.denoise(c_old, ybar.astype(np.float32), var.astype(np.float32), 5, 1, 1.0)[0]
    spread = ~np.isfinite(old).all(axis=-1)
    print(f"with the finite guide {int(spread.sum())} pixels come back non-finite")
    assert spread.sum() == 121
