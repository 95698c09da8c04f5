"""The denoising filter (rt_accum_denoise) without a GPU: the struct layout, the bindings, and properties of tests/denoise_ref.py, the numpy
restatement of the header's definition that the GPU tests hold the kernel to bit for bit."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import denoise_channels_ref
import denoise_ref
import test_denoise
import test_denoise_channels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_rtdenoise_layout_matches_the_c_compiler(rt, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x.h"\nint main(void){printf("%zu %zu %zu %zu %zu %u %u %.9g\\n",'
                   'sizeof(RtDenoise),offsetof(RtDenoise,radius),offsetof(RtDenoise,patch),offsetof(RtDenoise,strength),'
                   'offsetof(RtDenoise,reserved),RT_DENOISE_MAX_RADIUS,RT_DENOISE_MAX_PATCH,(double)RT_DENOISE_DEFAULT_STRENGTH);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    d, f = rt._ffi.RtDenoise, rt._ffi
    assert [int(x) for x in got[:5]] == [C.sizeof(d), d.radius.offset, d.patch.offset, d.strength.offset, d.reserved.offset] == [16, 0, 4, 8, 12]
    assert [int(x) for x in got[5:7]] == [f.DENOISE_MAX_RADIUS, f.DENOISE_MAX_PATCH] == [10, 3]
    assert F32(float(got[7])) == F32(f.DENOISE_DEFAULT_STRENGTH)


def test_the_denoise_entry_points_are_bound(rt):
    lib = rt._ffi.load_gpu_library()
    for name in ("rt_accum_denoise", "rt_debug_denoise"):
        assert name in rt._ffi.GPU_SYMBOLS and getattr(lib, name).restype is C.c_int
    for name in ("accum_denoise", "debug_denoise"):
        assert callable(getattr(rt.Renderer, name))
    assert rt.RtDenoise is rt._ffi.RtDenoise


def test_a_constant_image_without_variance_comes_back_bit_for_bit():
    # dyadic values: the sums of up to 121 equal terms (every weight is 1) are exact, so num / den returns the value itself
    c = np.broadcast_to(np.array([0.5, 0.25, 1.5], F32), (9, 14, 3)).copy()
    y, v = np.full((9, 14), 0.375, F32), np.zeros((9, 14), F32)
    out, shares = denoise_ref.denoise(c, y, v, 5, 1, 0.7)
    assert np.array_equal(_bits(out), _bits(c)) and shares == (0.0, 0.0, 1.0)


def test_a_nan_pixel_stays_itself_and_spreads_to_no_other():
    c, y, v = denoise_ref.kernel_case(21, 13)
    bad = ~np.isfinite(y)
    assert bad.sum() == 2 and np.isnan(y).sum() == 1
    for radius, patch in ((5, 1), (2, 3)):
        out, _ = denoise_ref.denoise(c, y, v, radius, patch, 0.7)
        assert np.array_equal(_bits(out[bad]), _bits(c[bad]))
        assert np.isfinite(out[~bad]).all()


def test_distinct_values_without_variance_are_not_averaged():
    rng = np.random.default_rng(3)
    c = rng.uniform(0.1, 2.0, (8, 11, 3)).astype(F32)
    y = (np.arange(88, dtype=F32).reshape(8, 11) + 1) / F32(16)  # distinct, at least 1/16 apart: (dy)^2 / eps is far beyond the support
    out, shares = denoise_ref.denoise(c, y, np.zeros_like(y), 4, 1, 1.0)
    assert np.array_equal(_bits(out), _bits(c))
    assert shares[1] == 0.0  # (only q = p has w = 1)
    n_pairs = sum((min(r + 4, 7) - max(r - 4, 0) + 1) * (min(x + 4, 10) - max(x - 4, 0) + 1) for r in range(8) for x in range(11))
    assert abs(shares[2] - 88 / n_pairs) < 1e-12


def test_the_result_is_a_function_of_the_neighbourhood_alone():
    """What lets a workgroup filter its tile from the tile plus a halo of radius + patch: a pixel's result depends on nothing farther away.
    A crop of the frame gives, for its pixels at least radius + patch from the cut, the bits the whole frame gives."""
    c, y, v = denoise_ref.kernel_case(37, 21)
    for radius, patch in ((3, 1), (2, 2)):
        h = radius + patch
        full, _ = denoise_ref.denoise(c, y, v, radius, patch, 0.45)
        y0, y1, x0, x1 = 2, 19, 5, 30
        part, _ = denoise_ref.denoise(c[y0:y1, x0:x1], y[y0:y1, x0:x1], v[y0:y1, x0:x1], radius, patch, 0.45)
        assert np.array_equal(_bits(part[h:-h, h:-h]), _bits(full[y0 + h:y1 - h, x0 + h:x1 - h]))
        assert (part[h:-h, h:-h] != c[y0 + h:y1 - h, x0 + h:x1 - h]).any()


# RMSE(filtered) / RMSE(noisy) against the truth, measured with denoise_ref on the seeded 64 x 48 frame at (R 5, F 1):
#   strength 0.45: 0.4155    0.7: 0.3498    1.0: 0.3197     (RMSE noisy 0.2440)
# The bound is the geometric mean of the measured ratio and 1: the input is seeded, the margin only guards later edits.
MEASURED = {0.45: 0.4155, 0.7: 0.3498, 1.0: 0.3197}


def test_the_filter_lowers_the_error_of_a_synthetic_frame():
    truth, c, y, v = denoise_ref.synthetic(64, 48)
    noisy = denoise_ref.rmse(c, truth)
    for k, ratio in MEASURED.items():
        got = denoise_ref.rmse(denoise_ref.denoise(c, y, v, 5, 1, k)[0], truth)
        print(f"strength {k}: RMSE {noisy:.4f} -> {got:.4f}, ratio {got / noisy:.4f}")
        assert got <= noisy * np.sqrt(ratio * 1.0)


def test_the_kernel_case_covers_every_weight_class():
    """The 37 x 21 (R 5, F 1) case of tests/test_denoise.py at its strength: each of w == 0, 0 < w < 1 and w == 1 holds at least 10 % of
    the pairs, so that a kernel that gets one class wrong cannot pass."""
    c, y, v = denoise_ref.kernel_case(37, 21)
    _, shares = denoise_ref.denoise(c, y, v, 5, 1, denoise_ref.KERNEL_CASE_STRENGTH)
    assert min(shares) >= 0.10, shares


# sha256 of out.tobytes() of (denoise_ref.denoise, denoise_channels_ref.denoise) on their kernel_case inputs at KERNEL_CASE_STRENGTH, for
# every entry of both KERNEL_CASES lists: computed with the two references as they were before they became wrappers of denoise_ref.nlm.
REFERENCE_DIGESTS = {
    (37, 21, 5, 1): ("be60f98af4410093fde2750072c6b3355fc8d3e8c4568bf65a15553863e5e783",
                     "48e970e4168dc77c97c8e0b505ce2b4ae358d5bb7a33335d009978ede8385dab"),
    (37, 21, 1, 0): ("4c01bbb29fa665650b84db9360b476789c3dd2587300668e920c64784a73ee0b",
                     "955ee1b02b2c07d68692be3e198bf93fa108fb46df073ea19ca4ae684d854997"),
    (13, 9, 10, 3): ("de7828c204373310e71ad40e2259295d379a53e6a3ee6d55fd542d6bde6cc00d",
                     "aa72f68bde8253be8aeba9ff5fd3603116afdbb6e0604e4b45a12b2c78b48ba1"),
    (1, 1, 5, 1): ("6b730b5f0d00d88b2f0abf3cb425f6a98644b3074a13e4b3507268eb6ef07d63",
                   "6b730b5f0d00d88b2f0abf3cb425f6a98644b3074a13e4b3507268eb6ef07d63"),
    (37, 21, 3, 2): ("e657eb97da4a1141e5df9a7feb67b71220764e1cf64630ef991ef0947cbc004a",
                     "90fe5e3d213c9b6244399ba4bdf1d93f34509aab3d34796517586dd5949a6014"),
    (17, 33, 2, 3): ("533ad64658cdf4eb1744ceeaf31e03d9327bb0a2a2025ee817a34aafaee4306f",
                     "8a6d016f39ac70490806a6aba60f4327e436016f8e551c4851ec105470bc824d"),
    (33, 17, 10, 3): ("ef4f664e2fca4fa027398c3e390df824a8a58f7792d695f464fd60b079e108e5",
                      "1da98278a9524a358b92739cab9622a1a9f20753e38ea4357eae591d464164be"),
}


def test_the_digests_cover_every_kernel_case():
    assert set(REFERENCE_DIGESTS) == set(test_denoise.KERNEL_CASES) == set(test_denoise_channels.KERNEL_CASES)


@pytest.mark.parametrize("case", list(REFERENCE_DIGESTS))
def test_the_folded_references_reproduce_the_digests_of_the_separate_ones(case):
    nx, rows, radius, patch = case
    k = denoise_ref.KERNEL_CASE_STRENGTH
    c, y, v = denoise_ref.kernel_case(nx, rows)
    c3, var3 = denoise_channels_ref.kernel_case(nx, rows)
    got = (hashlib.sha256(denoise_ref.denoise(c, y, v, radius, patch, k)[0].tobytes()).hexdigest(),
           hashlib.sha256(denoise_channels_ref.denoise(c3, var3, radius, patch, k)[0].tobytes()).hexdigest())
    assert got == REFERENCE_DIGESTS[case]


def test_the_plane_count_is_part_of_the_filter():
    """nlm with one guide plane is denoise_ref.denoise in bits; the same plane given three times is another filter (the term is the sum
    of three equal d, (d + d) + d, over three times the divisor: not d again in f32), so a fold that ignored the planes would show."""
    c, y, v = denoise_ref.kernel_case(37, 21)
    k = denoise_ref.KERNEL_CASE_STRENGTH
    one, shares = denoise_ref.nlm(c, [(y, v)], 5, 1, k)
    want, want_shares = denoise_ref.denoise(c, y, v, 5, 1, k)
    assert np.array_equal(_bits(one), _bits(want)) and shares == want_shares
    three, _ = denoise_ref.nlm(c, [(y, v)] * 3, 5, 1, k)
    assert three.shape == one.shape and not np.array_equal(_bits(three), _bits(one))
