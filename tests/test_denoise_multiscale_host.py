"""The multi-scale filter without a GPU: the new symbols and the struct layout against the C compiler, rt_denoise_level_size against the
reference, the defining properties of rtow_mi355x.h ("multi-scale denoising") on tests/denoise_multiscale_ref.py alone, one level against
both single-scale references in bits, the weight coverage of the coarse levels, the error on the synthetic frame, and
csrc/rt_multiscale_plan.h as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_channels_ref
import denoise_multiscale_ref as ref
import denoise_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ["rt_denoise_level_size", "rt_accum_denoise_multiscale", "rt_debug_denoise_multiscale"]
# (nx, rows, R, F) of tests/test_denoise_multiscale.py: the sizes at which an off-by-one of the odd-side tap, the border clamp of X' or the
# tile edge can show
CASES = [(37, 21, 5, 1), (37, 21, 1, 0), (13, 9, 10, 3), (1, 1, 5, 1), (2, 2, 5, 1), (3, 1, 2, 1), (1, 5, 2, 0), (17, 33, 2, 3), (33, 17, 10, 3),
         (35, 19, 3, 2)]
K = denoise_ref.KERNEL_CASE_STRENGTH


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()), "values differ")


def test_symbols_and_struct_layout_match_the_c_compiler(rt, tmp_path):
    f = rt._ffi
    lib = f.load_gpu_library()
    assert lib.rt_abi_version() == 11 == f.EXPECTED_ABI  # only symbols and one struct were added
    for n in NEW_SYMBOLS:
        assert n in f.GPU_SYMBOLS and hasattr(lib, n), n
    names = [n for n, _ in f.RtMultiscale._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x_debug.h"\n'
                   'int main(void){int (*a)(uint32_t, uint32_t, uint32_t, uint32_t*, uint32_t*) = rt_denoise_level_size;\n'
                   'int (*b)(RtCtx*, const RtDenoise*, const RtMultiscale*, float*, uint8_t*) = rt_accum_denoise_multiscale;\n'
                   'int (*c)(RtCtx*, uint32_t, uint32_t, uint32_t, const float*, const float*, const float*, const RtDenoise*, uint32_t, float*,'
                   ' uint32_t, float*, float*, float*) = rt_debug_denoise_multiscale;\n'
                   'printf("%zu' + " %zu" * len(names) + ' %d %u %u %u %u %u\\n", sizeof(RtMultiscale), ' +
                   ", ".join("offsetof(RtMultiscale, %s)" % n for n in names) +
                   ', (a != 0) + (b != 0) + (c != 0), RT_DENOISE_MAX_LEVELS, RT_DENOISE_DEFAULT_LEVELS, RT_DENOISE_GUIDE_LUMINANCE,'
                   ' RT_DENOISE_GUIDE_CHANNELS, RT_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", os.path.dirname(f.GPU_LIB_PATH),
                    "-l:librtow_mi355x.so", "-Wl,-rpath," + os.path.dirname(f.GPU_LIB_PATH), "-Wl,--allow-shlib-undefined"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    M = f.RtMultiscale
    assert got == [C.sizeof(M)] + [getattr(M, n).offset for n in names] + [3, f.DENOISE_MAX_LEVELS, f.DENOISE_DEFAULT_LEVELS, f.DENOISE_GUIDE_LUMINANCE,
                                                                            f.DENOISE_GUIDE_CHANNELS, 11]
    assert names == ["levels", "guide", "reserved"] and C.sizeof(M) == 16
    assert f.DENOISE_MAX_LEVELS == ref.MAX_LEVELS == 4 and 1 <= f.DENOISE_DEFAULT_LEVELS <= 4


def test_level_sizes_of_the_library_against_the_reference(rt):
    lib = rt._ffi.load_gpu_library()
    a, b = C.c_uint32(), C.c_uint32()
    for nx in range(1, 71):
        for rows in (1, 2, 3, nx, 71 - nx):
            for level in range(ref.MAX_LEVELS):
                assert lib.rt_denoise_level_size(nx, rows, level, C.byref(a), C.byref(b)) == 0
                assert (a.value, b.value) == ref.level_size(nx, rows, level) == rt.denoise_level_size(nx, rows, level), (nx, rows, level)
    assert ref.level_size(70, 1, 3) == (9, 1) and ref.level_size(5, 5, 3) == (1, 1) and ref.level_size(1, 1, 3) == (1, 1)
    inv = -rt._ffi.ERR_INVALID
    assert lib.rt_denoise_level_size(0, 4, 0, None, None) == inv and lib.rt_denoise_level_size(4, 0, 0, None, None) == inv
    assert lib.rt_denoise_level_size(4, 4, ref.MAX_LEVELS, None, None) == inv and lib.rt_denoise_level_size(4, 4, 0, None, None) == 0
    assert lib.rt_denoise_level_size(2 ** 32 - 1, 2 ** 32 - 2, 1, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (2 ** 31, 2 ** 31 - 1)


# ---- the pieces -----------------------------------------------------------------------------------------------------------------------
def test_down_counts_the_taps_inside():
    """D on hand-made planes: 5 x 3 has k = 4, 2 (last column), 2 (last row) and 1 (the corner)."""
    a = np.arange(15, dtype=F32).reshape(3, 5)
    mean, var = ref.down(a), ref.down(a, variance=True)
    assert mean.shape == (2, 3) == var.shape
    assert mean.tolist() == [[(0 + 1 + 5 + 6) / 4, (2 + 3 + 7 + 8) / 4, (4 + 9) / 2], [(10 + 11) / 2, (12 + 13) / 2, 14.0]]
    assert var.tolist() == [[(0 + 1 + 5 + 6) / 16, (2 + 3 + 7 + 8) / 16, (4 + 9) / 4], [(10 + 11) / 4, (12 + 13) / 4, 14.0]]
    rgb = np.stack([a, a + 1, a * 2], axis=-1)
    _same(ref.down(rgb)[..., 2], ref.down(a * 2), "an image is its planes")
    one = np.array([[F32(0.3)]])
    _same(ref.down(one), one, "1 x 1 stays")
    _same(ref.down(one, variance=True), one, "1 x 1 stays, variance")


def test_up_add_is_the_bilinear_interpolation_clamped_at_the_border():
    e = np.zeros((2, 3, 3), F32)
    e[0, 1] = 16.0
    got = ref.up_add(np.zeros((3, 5, 3), F32), e)[..., 0]
    # x: 0 1 | 2 3 | 4 over X = 0, 1, 2; pixel 2 looks at X' = 0, pixel 3 at X' = 2, pixel 1 at X' = 1, pixel 4 at X' = 1
    # y: 0 1 | 2 over Y = 0, 1; row 0 looks at Y' = 0 (clamped), row 1 at Y' = 1, row 2 at Y' = 0
    assert got.tolist() == [[0.0, 4.0, 12.0, 12.0, 4.0], [0.0, 3.0, 9.0, 9.0, 3.0], [0.0, 1.0, 3.0, 3.0, 1.0]]
    flat = np.full((4, 6, 3), F32(0.7))
    _same(ref.up_add(np.zeros((7, 11, 3), F32), flat), np.full((7, 11, 3), F32(0.7)), "a constant e is added as it is")


# ---- the four properties of the header ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,rows,radius,patch", CASES)
def test_one_level_is_the_single_scale_filter_of_the_guide(nx, rows, radius, patch):
    c, y, v = denoise_ref.kernel_case(nx, rows)
    _same(ref.luminance(c, y, v, radius, patch, K, 1)[0], denoise_ref.denoise(c, y, v, radius, patch, K)[0], "luminance")
    c3, var3 = denoise_channels_ref.kernel_case(nx, rows)
    _same(ref.channels(c3, var3, radius, patch, K, 1)[0], denoise_channels_ref.denoise(c3, var3, radius, patch, K)[0], "channels")


@pytest.mark.parametrize("levels", [2, 3, 4])
@pytest.mark.parametrize("guide", ["luminance", "channels"])
def test_a_non_finite_pixel_stays_itself_and_spreads_to_no_other(guide, levels):
    """The NaN and the +inf pixel of kernel_case come back as they are and every other pixel is finite; a finite sibling of theirs under
    the same coarse pixel gets its level-0 result, the e of that coarse pixel being 0."""
    nx, rows = 37, 21
    if guide == "luminance":
        c, y, v = denoise_ref.kernel_case(nx, rows)
        out, lv = ref.luminance(c, y, v, 5, 1, K, levels)
    else:
        c, var = denoise_channels_ref.kernel_case(nx, rows)
        out, lv = ref.channels(c, var, 5, 1, K, levels)
    bad = ~np.isfinite(c).all(axis=-1)
    assert bad.sum() == 2 and bad[1, nx - 2] and bad[rows - 2, 1]
    _same(out[bad], c[bad], "the non-finite pixels")
    assert np.isfinite(out[~bad]).all()
    for s in range(1, levels):
        assert (~np.isfinite(lv[s]["c"]).all(axis=-1)).sum() == 2, ("one coarse pixel per non-finite pixel", s)
    assert (lv[0]["e"][0, (nx - 2) // 2] == 0).all() and (lv[0]["e"][(rows - 2) // 2, 0] == 0).all()
    # (35, 0) lies under the coarse pixel (17, 0) of the NaN (35, 1), in the corner of its quadrant that looks at the row below, clamped to
    # itself, and at the coarse column 18, so it keeps F_0 plus only what column 18 gives
    sibling = (0, nx - 2)
    e = lv[0]["e"]
    want = lv[0]["F"][sibling] + ((ref.W_NEAR * e[0, 17] + ref.W_SIDE * e[0, 18]) + (ref.W_SIDE * e[0, 17] + ref.W_FAR * e[0, 18]))
    _same(out[sibling], want.astype(F32), "a finite sibling")
    assert np.isfinite(out[sibling]).all()


@pytest.mark.parametrize("guide", ["luminance", "channels"])
@pytest.mark.parametrize("nx,rows", [(16, 8), (13, 9), (1, 1), (3, 1)])
def test_a_constant_dyadic_image_without_variance_comes_back(guide, nx, rows):
    c = np.empty((rows, nx, 3), F32)
    c[...] = [0.5, 0.25, 0.75]
    zero = np.zeros((rows, nx), F32)
    for levels in range(1, ref.MAX_LEVELS + 1):
        if guide == "luminance":
            out, _ = ref.luminance(c, np.full((rows, nx), F32(0.375)), zero, 5, 1, 1.0, levels)
        else:
            out, _ = ref.channels(c, np.zeros_like(c), 5, 1, 1.0, levels)
        _same(out, c, (guide, nx, rows, levels))


def test_the_inputs_are_read_and_not_changed():
    c, y, v = denoise_ref.kernel_case(35, 19)
    kept = [a.copy() for a in (c, y, v)]
    out, lv = ref.luminance(c, y, v, 3, 2, K, 3)
    for a, b in zip((c, y, v), kept):
        _same(a, b, "an input")
    assert [l["c"].shape[:2] for l in lv] == [(19, 35), (10, 18), (5, 9)] and out.dtype == F32
    again, _ = ref.luminance(c, y, v, 3, 2, K, 3)
    _same(again, out, "a second run")


@pytest.mark.parametrize("nx,rows,radius,patch", CASES)
def test_levels_matter_on_every_case(nx, rows, radius, patch):
    """A call that ignores `levels` fails the GPU test: on every case but 1 x 1 two levels and more differ from one in most pixels."""
    c, y, v = denoise_ref.kernel_case(nx, rows)
    one = ref.luminance(c, y, v, radius, patch, K, 1)[0]
    for levels in (2, 3, 4):
        out = ref.luminance(c, y, v, radius, patch, K, levels)[0]
        differ = int((_bits(out) != _bits(one)).any(axis=-1).sum())
        if (nx, rows) == (1, 1):
            assert differ == 0  # D of one pixel is the pixel, e = 0
        else:
            assert differ >= min(93, nx * rows // 2), (nx, rows, levels, differ)


# ---- the weight coverage of the coarse levels -----------------------------------------------------------------------------------------
def test_weight_coverage_of_the_coarse_levels():
    """A coarse level has a quarter of the variance, so most pairs there have weight 0: the 37 x 21 case still puts at least 10 % of the
    pairs of level 1 in each weight class at (R 5, F 1), and leaves no class empty at level 2 with (R 1, F 0)."""
    c, y, v = denoise_ref.kernel_case(37, 21)
    shares = ref.luminance(c, y, v, 5, 1, K, 2)[1][1]["shares"]
    print("level 1, (R 5, F 1): w == 0, 0 < w < 1, w == 1:", shares)
    assert min(shares) >= 0.10, shares
    assert [round(x, 2) for x in shares] == [0.73, 0.14, 0.13]
    shares = ref.luminance(c, y, v, 1, 0, K, 3)[1][2]["shares"]
    print("level 2, (R 1, F 0):", shares)
    assert min(shares) > 0.0, shares
    assert [round(x, 2) for x in shares] == [0.52, 0.08, 0.40]


# ---- quality on the synthetic frame ---------------------------------------------------------------------------------------------------
# RMSE(filtered) / RMSE(noisy) against the truth for 1, 2 and 3 levels, strength 1.0, patch 1: the figures the definition was accepted on
QUALITY = [((64, 48, 16, 7), 5, (0.3197, 0.2818, 0.2847)), ((64, 48, 16, 7), 3, (0.3218, 0.2937, 0.2934))]


@pytest.mark.parametrize("frame,radius,ratios", QUALITY)
def test_quality_on_the_synthetic_frame(frame, radius, ratios):
    nx, rows, n, seed = frame
    truth, c, y, v = denoise_ref.synthetic(nx, rows, n=n, seed=seed)
    noisy = denoise_ref.rmse(c, truth)
    got = [denoise_ref.rmse(ref.luminance(c, y, v, radius, 1, 1.0, levels)[0], truth) / noisy for levels in (1, 2, 3)]
    print(frame, radius, ["%.4f" % x for x in got])
    assert [round(x, 4) for x in got] == list(ratios), "the reference and the accepted figures disagree: the definition is not the one that was measured"
    assert got[1] < got[0]
    if radius == 5:
        assert got[1] * noisy <= noisy * np.sqrt(ratios[1] * 1.0)


# ---- csrc/rt_multiscale_plan.h under the sanitizers -----------------------------------------------------------------------------------
def test_multiscale_plan_header_under_asan_ubsan(tmp_path):
    """csrc/rt_multiscale_plan.h compiled into tests/multiscale_plan_main.cpp with AddressSanitizer + UBSan: every section made its
    checks, none failed and no sanitizer reported."""
    exe = str(tmp_path / "multiscale_plan_san")
    c = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-Wall", "-Wextra",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray_tracing_in_one_weekend_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "multiscale_plan_main.cpp")], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l[0] for l in lines] == ["sizes", "check", "plan", "ok"]
    assert all(int(l[1]) > 0 for l in lines[:-1])
