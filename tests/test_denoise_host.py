"""The denoising filter (rt_accum_denoise) without a GPU: the struct layout, the bindings, and properties of tests/denoise_ref.py, the numpy
restatement of the header's definition that the GPU tests hold the kernel to bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

import denoise_ref

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
