"""Channel moments and the colour-guided filter (rt_accum_track_channels, rt_accum_denoise_channels) without a GPU: the bindings, the
unchanged struct layouts, and properties of tests/denoise_channels_ref.py, the numpy restatement of the header's definition that the GPU
tests hold the kernels to bit for bit."""
import ctypes as C

import numpy as np

import denoise_channels_ref as ch_ref
import denoise_ref
import noise_ref

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_the_entry_points_are_bound_and_the_structs_unchanged(rt):
    f = rt._ffi
    lib = f.load_gpu_library()
    for name in ("rt_accum_track_channels", "rt_accum_read_channel_sem", "rt_accum_denoise_channels", "rt_debug_denoise_channels"):
        assert name in f.GPU_SYMBOLS and getattr(lib, name).restype is C.c_int, name
    for name in ("accum_track_channels", "accum_channel_sem", "accum_denoise_channels", "debug_denoise_channels"):
        assert callable(getattr(rt.Renderer, name)), name
    d = f.RtDenoise
    assert [C.sizeof(d), d.radius.offset, d.patch.offset, d.strength.offset, d.reserved.offset] == [16, 0, 4, 8, 12]
    assert C.sizeof(f.RtNoise) == 32 and C.sizeof(f.RtAdaptive) == 24 and C.sizeof(f.RtAdaptiveInfo) == 24
    assert lib.rt_abi_version() == 11 == f.EXPECTED_ABI


def test_a_constant_image_without_variance_comes_back_bit_for_bit():
    # dyadic values: the sums of up to 121 equal terms (every weight is 1) are exact, so num / den returns the value itself
    c = np.broadcast_to(np.array([0.5, 0.25, 1.5], F32), (9, 14, 3)).copy()
    out, shares = ch_ref.denoise(c, np.zeros_like(c), 5, 1, 0.7)
    assert np.array_equal(_bits(out), _bits(c)) and shares == (0.0, 0.0, 1.0)


def test_a_nan_pixel_stays_itself_and_spreads_to_no_other():
    c, var = ch_ref.kernel_case(21, 13)
    bad = ~np.isfinite(c).all(axis=-1)
    assert bad.sum() == 2 and np.isnan(c[..., 0]).sum() == 1 and np.isinf(c[..., 0]).sum() == 1
    for radius, patch in ((5, 1), (2, 3)):
        out, _ = ch_ref.denoise(c, var, radius, patch, 0.7)
        assert np.array_equal(_bits(out[bad]), _bits(c[bad]))
        assert np.isfinite(out[~bad]).all()


def test_two_colours_of_equal_luminance_are_not_averaged():
    """The property in its smallest form.  Left half red (1, 0, 0), right half the green (0, 0.2126 / 0.7152, 0) of the same Rec. 709
    luminance (to an ulp of f32); no pixel has any variance.  The luminance-guided reference sees one flat image and averages the two
    colours; the channel-guided one returns the image."""
    c = np.zeros((4, 6, 3), F32)
    c[:, :3], c[:, 3:] = [1.0, 0.0, 0.0], [0.0, 0.2126 / 0.7152, 0.0]
    y = noise_ref.luminance(c).astype(F32)
    assert np.abs(y - F32(0.2126)).max() < 2e-8
    zero = np.zeros((4, 6), F32)
    by_luminance, _ = denoise_ref.denoise(c, y, zero, 3, 1, 1.0)
    by_channels, shares = ch_ref.denoise(c, np.zeros_like(c), 3, 1, 1.0)
    # (the green is not dyadic: num / den of up to 28 equal terms may round it by an ulp; that is all that may happen)
    assert np.abs(by_channels - c).max() <= 6e-8
    assert np.abs(by_luminance - c).max(axis=-1).min() > 0.05, "every pixel is within three columns of the edge and takes colour from across it"
    assert shares[1] == 0.0 and 0.0 < shares[0] < 1.0  # weights are 0 or 1 only


# The banded frame (ch_ref.truth_bands), 64 x 48, seed 7, n = 64, R 5, F 1, strength 1.0, measured with the references here:
#   RMSE noisy 0.14309, luminance-guided 0.11782, channel-guided 0.03966;   on the banded half alone 0.12913, 0.15582, 0.02983.
# MEASURED_RATIO = channel-guided / luminance-guided; the bound is the geometric mean of the measured ratio and 1, as in
# test_denoise_host.py: the input is seeded, the margin only guards later edits.
MEASURED_RATIO = 0.3366


def test_the_banded_frame():
    tb, half = ch_ref.truth_bands(64, 48)
    lum = ch_ref.luminance709(tb[half])
    assert abs(lum - ch_ref.BAND_LUMINANCE).max() < 1e-6 and len(np.unique(tb[half].reshape(-1, 3), axis=0)) == 4
    truth, c, y, v, var = ch_ref.synthetic_channels(64, 48, 64, 7, truth=tb)
    by_luminance = denoise_ref.denoise(c, y, v, 5, 1, 1.0)[0]
    by_channels = ch_ref.denoise(c, var, 5, 1, 1.0)[0]
    e = [denoise_ref.rmse(a, truth) for a in (c, by_luminance, by_channels)]
    eh = [denoise_ref.rmse(a[half], truth[half]) for a in (c, by_luminance, by_channels)]
    print("banded frame: noisy %.5f luminance-guided %.5f channel-guided %.5f; banded half: %.5f %.5f %.5f" % (*e, *eh))
    assert e[2] < e[0]
    assert e[2] <= e[1] * np.sqrt(MEASURED_RATIO * 1.0)
    assert eh[1] > eh[0], "the defect this filter removes: on equal-luminance edges the luminance-guided filter leaves more error than it got"


def test_the_standard_frame_is_filtered_as_well_as_by_luminance():
    # measured: strength 0.7: 0.08442 against 0.08535, 1.0: 0.07799 against 0.07800 (RMSE noisy 0.24400)
    truth, c, y, v, var = ch_ref.synthetic_channels(64, 48, 16, 7)
    ref = denoise_ref.synthetic(64, 48, 16, 7)
    assert np.array_equal(_bits(c), _bits(ref[1])) and np.array_equal(_bits(v), _bits(ref[3]))  # the same frame
    for k in (0.7, 1.0):
        by_luminance = denoise_ref.rmse(denoise_ref.denoise(c, y, v, 5, 1, k)[0], truth)
        by_channels = denoise_ref.rmse(ch_ref.denoise(c, var, 5, 1, k)[0], truth)
        print(f"strength {k}: luminance-guided {by_luminance:.5f}, channel-guided {by_channels:.5f}")
        assert abs(by_channels - by_luminance) <= 0.05 * by_luminance


def test_the_kernel_case_covers_every_weight_class_and_its_special_pixels():
    c, var = ch_ref.kernel_case(37, 21)
    _, shares = ch_ref.denoise(c, var, 5, 1, ch_ref.KERNEL_CASE_STRENGTH)
    assert min(shares) >= 0.10, shares
    zero = var == 0
    assert zero.all(axis=-1).sum() >= 8 and (zero.sum(axis=-1) == 1).sum() >= 1


def test_the_replay_of_the_moments_takes_counts_per_pixel():
    rng = np.random.default_rng(5)
    frames = [rng.uniform(0, 2, (3, 4, 3)).astype(F32) for _ in range(6)]
    counts = rng.integers(0, 7, (3, 4)).astype(np.uint32)
    counts[0, 0], counts[0, 1] = 0, 1
    s1, s2 = ch_ref.accumulate_channels(frames, counts)
    v = ch_ref.channel_variance(s1, s2, counts)
    for (j, i), n in np.ndenumerate(counts):
        a1, a2 = ch_ref.accumulate_channels([f[j:j + 1, i:i + 1] for f in frames[:n]] or [np.zeros((1, 1, 3), F32)])
        if n == 0:
            a1, a2 = a1 * 0, a2 * 0
        assert np.array_equal(s1[j, i], a1[0, 0]) and np.array_equal(s2[j, i], a2[0, 0])
        assert np.array_equal(v[j, i], ch_ref.channel_variance(a1, a2, int(n))[0, 0])
    assert (v[0, 0] == 0).all() and (v[0, 1] == 0).all()
