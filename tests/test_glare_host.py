"""The glare without a GPU: the new symbols and struct layouts against the C compiler, every refusal of rt_glare_check through ctypes,
csrc/rt_glare_plan.h as a stand-alone program under AddressSanitizer + UBSan, and the properties the header states — proved on
tests/glare_ref.py alone: the weights, a constant image, the energy of an interior impulse and of the corner impulses, out >= 0,
amount == 0 under the reference quantisation, the threshold's edge, inputs at FLT_MAX and around 2^64, and the share of ambiguous sRGB
values on the planes the GPU test uses."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
import display_ref
import glare_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def test_symbols_and_struct_layouts_match_the_c_compiler(rt, tmp_path):
    f = rt._ffi
    lib = f.load_gpu_library()
    for n in ("rt_set_glare", "rt_glare_check", "rt_glare_info", "rt_glare_image", "rt_debug_glare", "rt_debug_glare_chain"):
        assert n in f.GPU_SYMBOLS and hasattr(lib, n), n
    gf, inf_ = [n for n, _ in f.RtGlare._fields_], [n for n, _ in f.RtGlareInfo._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x_debug.h"\n'
                   'int main(void){int (*a)(RtCtx*, const RtGlare*) = rt_set_glare;\n'
                   'int (*b)(const RtGlare*) = rt_glare_check;\n'
                   'int (*c)(RtCtx*, RtGlareInfo*) = rt_glare_info;\n'
                   'int (*d)(RtCtx*, float*) = rt_glare_image;\n'
                   'int (*e)(RtCtx*, uint32_t, uint32_t, const float*, const RtGlare*, const RtDisplay*, float*, uint8_t*, RtGlareInfo*) = rt_debug_glare;\n'
                   'int (*g)(RtCtx*, uint32_t) = rt_debug_glare_chain;\n'
                   'printf("%zu' + " %zu" * (len(gf) + 1 + len(inf_)) + ' %d %u %u %.9g %.9g %u %u %u %u\\n", sizeof(RtGlare), ' +
                   ", ".join("offsetof(RtGlare, %s)" % n for n in gf) + ", sizeof(RtGlareInfo), " +
                   ", ".join("offsetof(RtGlareInfo, %s)" % n for n in inf_) +
                   ', (a != 0) + (b != 0) + (c != 0) + (d != 0) + (e != 0) + (g != 0), RT_GLARE_MAX_LEVELS, RT_GLARE_DEFAULT_LEVELS,'
                   ' (double)RT_GLARE_DEFAULT_AMOUNT, (double)RT_GLARE_DEFAULT_SPREAD, RT_GLARE_CHAIN_AUTO, RT_GLARE_CHAIN_PLAIN, RT_GLARE_CHAIN_FUSED,'
                   ' RT_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", os.path.dirname(f.GPU_LIB_PATH),
                    "-l:librtow_mi355x.so", "-Wl,-rpath," + os.path.dirname(f.GPU_LIB_PATH), "-Wl,--allow-shlib-undefined"], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    G, I = f.RtGlare, f.RtGlareInfo
    want = [C.sizeof(G)] + [getattr(G, n).offset for n in gf] + [C.sizeof(I)] + [getattr(I, n).offset for n in inf_]
    assert [int(x) for x in got[:len(want)]] == want and (C.sizeof(G), C.sizeof(I)) == (16, 16)
    rest = got[len(want):]
    assert [int(rest[0]), int(rest[1]), int(rest[2])] == [6, f.GLARE_MAX_LEVELS, f.GLARE_DEFAULT_LEVELS] and f.GLARE_MAX_LEVELS == ref.MAX_LEVELS == 8
    assert F32(rest[3]) == F32(f.GLARE_DEFAULT_AMOUNT) and F32(rest[4]) == F32(f.GLARE_DEFAULT_SPREAD) and f.GLARE_DEFAULT_LEVELS == 6
    assert [int(x) for x in rest[5:8]] == [f.GLARE_CHAIN_AUTO, f.GLARE_CHAIN_PLAIN, f.GLARE_CHAIN_FUSED] and int(rest[8]) == 11
    assert gf == ["amount", "spread", "threshold", "levels"] and inf_ == ["levels", "coarse_nx", "coarse_rows", "reserved"]
    g = rt.make_glare()
    assert (g.amount, g.spread, g.threshold, g.levels) == (F32(f.GLARE_DEFAULT_AMOUNT), F32(f.GLARE_DEFAULT_SPREAD), 0.0, 6)


def test_glare_check_names_every_refusal(rt):
    assert not rt.glare_check(None)
    good = dict(amount=0.25, spread=0.5, threshold=1.0, levels=3)
    assert rt.glare_check(rt.make_glare(**good)) and rt.glare_check(rt.make_glare())
    nan, inf = float("nan"), float("inf")
    for field in ("amount", "spread", "threshold"):
        assert not rt.glare_check(rt.make_glare(**dict(good, **{field: nan}))), field
    for a in (-1e-6, float(np.nextafter(F32(1), F32(2))), 2.0, inf, -inf):
        assert not rt.glare_check(rt.make_glare(**dict(good, amount=a))), a
    for a in (0.0, 1.0):
        assert rt.glare_check(rt.make_glare(**dict(good, amount=a))), a
    for s in (0.0, -0.5, float(np.nextafter(F32(1), F32(2))), inf, -inf):
        assert not rt.glare_check(rt.make_glare(**dict(good, spread=s))), s
    for s in (1.0, 1e-45):
        assert rt.glare_check(rt.make_glare(**dict(good, spread=s))), s
    for t in (-1e-45, -1.0, inf, -inf):
        assert not rt.glare_check(rt.make_glare(**dict(good, threshold=t))), t
    for t in (0.0, float(np.finfo(F32).max)):
        assert rt.glare_check(rt.make_glare(**dict(good, threshold=t))), t
    for l in (0, 9, 0xFFFFFFFF):
        assert not rt.glare_check(rt.make_glare(**dict(good, levels=l))), l
    for l in range(1, 9):
        assert rt.glare_check(rt.make_glare(**dict(good, levels=l))), l


def test_glare_plan_header_under_asan_ubsan(tmp_path):
    """csrc/rt_glare_plan.h compiled into tests/glare_plan_main.cpp with AddressSanitizer + UBSan: every section made its checks, none
    failed and no sanitizer reported."""
    exe = str(tmp_path / "glare_plan_san")
    c = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-Wall", "-Wextra",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray_tracing_in_one_weekend_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "glare_plan_main.cpp")], capture_output=True, text=True, timeout=600)
    if c.returncode != 0 and "sanitize" in c.stderr + c.stdout and "cannot find" in c.stderr + c.stdout:
        pytest.skip("sanitizer runtime not available")
    assert c.returncode == 0, c.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l[0] for l in lines] == ["check", "levels", "weights", "layout", "ok"]
    assert all(int(l[1]) > 0 for l in lines[:-1])


def test_effective_levels_and_sizes():
    want = {(1, 1): (0, 1, 1), (1, 9): (4, 1, 1), (5, 1): (3, 1, 1), (2, 2): (1, 1, 1), (7, 13): (4, 1, 1), (33, 17): (6, 1, 1), (64, 64): (6, 1, 1),
            (257, 129): (8, 2, 1), (300, 200): (8, 2, 1)}
    for (nx, rows) in ref.FRAMES:
        _, info = ref.glare(np.zeros((rows, nx, 3), F32), ref.make(levels=8))
        assert (info["levels"], info["coarse_nx"], info["coarse_rows"]) == want[(nx, rows)], (nx, rows)
        assert ref.effective_levels(nx, rows, 3) == min(3, want[(nx, rows)][0])
    sizes = [ref.ms.level_size(257, 129, l) for l in range(9)]
    assert all(nx % 2 == 1 for nx, _ in sizes[:8]) and sizes[8] == (2, 1)  # odd at every level


def test_weights_sum_to_one_within_le_ulp():
    for spread, le in itertools.product((1.0, 0.7, 0.5, 0.1, 1e-3), range(1, 9)):
        w = ref.weights(F32(spread), le)
        assert all(v.dtype == F32 and v > 0 for v in w) and all(a >= b for a, b in zip(w, w[1:]))
        assert abs(sum(float(v) for v in w) - 1.0) <= le * 2.0 ** -24, (spread, le)
    assert ref.weights(F32(0.3), 1) == [F32(1)] and ref.weights(F32(1), 4) == [F32(0.25)] * 4


def test_constant_image_stays_that_constant():
    """Against the f64 evaluation, which keeps the constant to f64's rounding, within the bound of glare_ref.rounding_bound."""
    for (nx, rows), (a, sp, L) in itertools.product(ref.FRAMES, ((0.25, 0.5, 8), (1.0, 0.7, 3), (1.0, 1.0, 8))):
        c = ref.constant_plane(nx, rows)
        g = ref.make(a, sp, 0.0, L)
        out, info = ref.glare(c, g)
        o64 = ref.glare64(c, g)
        assert np.abs(o64 / c - 1).max() <= 1e-13, (nx, rows)
        err = np.abs(out.astype(F64) - o64)
        bound = ref.rounding_bound(info["levels"]) * (o64 + c)
        print(nx, rows, a, sp, L, "largest relative deviation", float(np.abs(out / c - 1).max()), "bound", 2 * ref.rounding_bound(info["levels"]))
        assert (err <= bound).all(), (nx, rows, a, sp, L, float((err / bound).max()))


def test_energy_of_an_interior_impulse_is_conserved():
    """256 x 256 (a multiple of 2^Le), threshold 0, an impulse 64 = 2^(5+1) pixels and more from every edge: the f64 evaluation conserves
    the energy to f64's rounding, the f32 one within twice the per-value bound (sum |error| <= R (sum out + sum s) = 2 R E)."""
    for L, pos in itertools.product((1, 3, 5), ((64, 64), (100, 77), (191, 191), (127, 128))):
        img = np.zeros((256, 256, 3), F32)
        img[pos] = (1000.0, 600.0, 250.0)
        g = ref.make(0.25, 0.7, 0.0, L)
        out, info = ref.glare(img, g)
        assert info["levels"] == L and min(pos) >= 2 ** (L + 1) and 255 - max(pos) >= 2 ** (L + 1)
        E = img.astype(F64).sum(axis=(0, 1))
        e64, e32 = ref.glare64(img, g).sum(axis=(0, 1)), out.astype(F64).sum(axis=(0, 1))
        print(L, pos, "relative energy error f64", (e64 / E - 1), "f32", (e32 / E - 1))
        assert (np.abs(e64 / E - 1) <= 1e-13).all()
        assert (np.abs(e32 / E - 1) <= 2 * ref.rounding_bound(L)).all(), (L, pos, e32 / E - 1)
        assert (out[pos] < img[pos]).all() and (out >= 0).all() and np.count_nonzero(out[..., 0]) > 1


def test_corner_impulses_are_held_to_the_f64_evaluation_not_to_one():
    """53 x 37 under the default glare: the border rule lets the odd corner (the last row and column, alone in their coarse pixels at
    several levels) gain energy and the even corner lose a little; the f32 reference agrees with the f64 evaluation of the same formulas."""
    g = ref.make()
    gains = {}
    for pos in ((0, 0), (0, 52), (36, 0), (36, 52)):
        img = np.zeros((37, 53, 3), F32)
        img[pos] = 1.0
        out, info = ref.glare(img, g)
        o64 = ref.glare64(img, g)
        e32, e64 = out.astype(F64).sum() / 3, o64.sum() / 3
        gains[pos] = e64 - 1
        assert abs(e32 - e64) <= ref.rounding_bound(info["levels"]) * (e64 + 1), (pos, e32, e64)
        assert (np.abs(out.astype(F64) - o64) <= ref.rounding_bound(info["levels"]) * (o64 + img)).all()
    print("energy gained by a corner impulse of a 53 x 37 frame under the default glare:", gains)
    assert 0.5 < gains[(36, 52)] < 1.0 and -0.01 < gains[(0, 0)] < 0.0  # (+70 % and -0.4 %: the consequence the header documents)


def test_out_is_not_negative_where_the_input_is_finite():
    for (nx, rows), (a, sp, t, L) in itertools.product(ref.FRAMES, ((1.0, 1.0, 0.0, 8), (1.0, 0.5, 1.0, 3), (0.25, 0.7, 0.0, 1))):
        c = ref.random_plane(nx, rows)
        out, _ = ref.glare(c, ref.make(a, sp, t, L))
        fin = np.isfinite(c).all(axis=-1)
        assert (out[fin] >= 0).all() and np.isfinite(out[fin]).all(), (nx, rows)
        assert np.array_equal(out[~fin].view(np.uint32), c[~fin].view(np.uint32)), (nx, rows)  # passed through unchanged, finite neighbours or not
        if nx * rows > 64:
            assert (~fin).sum() >= 3 and (c < 0).any() and (c > ref.CEILING).any()


def test_amount_zero_is_no_glare_under_the_reference_quantisation():
    """On the quantisation planes (either side of every step of the reference quantisation, the special bit patterns, NaN and the
    infinities among them): out differs from c only where c < 0, c > 2^64 or c is -0, and out_rgb8 not at all."""
    for (nx, rows) in ((7, 5), (64, 3), (300, 220)):
        c = display_ref.designed_plane(nx, rows)
        for sp, t, L in ((0.7, 0.0, 6), (1.0, 0.5, 8)):
            out, _ = ref.glare(c, ref.make(0.0, sp, t, L))
            assert np.array_equal(denoise_ref.finalize_rgb8(out), denoise_ref.finalize_rgb8(c))
            assert np.array_equal(display_ref.display(out, display_ref.make())[0], denoise_ref.finalize_rgb8(c))
            same = out.view(np.uint32) == c.view(np.uint32)
            with np.errstate(invalid="ignore"):
                fin = np.isfinite(c).all(axis=-1, keepdims=True)
                assert (same | (fin & ((c < 0) | (c > ref.CEILING) | ((c == 0) & np.signbit(c))))).all()
            assert nx * rows < 1000 or not same.all()  # (the large frame holds all of designed_pixels: negatives, FLT_MAX and -0 too)


def test_the_threshold_edge():
    c = np.zeros((9, 11, 3), F32)
    c[4, 5] = (0.8, 2.0, 0.3)
    Y = display_ref.luminance(c)[4, 5]
    at, _ = ref.glare(c, ref.make(0.5, 0.7, Y, 3))  # Y == threshold exactly: nothing is added
    assert np.array_equal(at.view(np.uint32), c.view(np.uint32))
    above, info = ref.glare(c, ref.make(0.5, 0.7, np.nextafter(Y, F32(0)), 3))  # Y the next f32 above the threshold: something is
    assert info["b"][4, 5].max() > 0 and np.count_nonzero(above[..., 1]) > 1 and (above[4, 5] <= c[4, 5]).all() and (above[4, 5] < c[4, 5]).any()
    # a frame wholly under the threshold is s
    r = ref.random_plane(33, 17)
    r = np.where(np.isfinite(r), np.minimum(r, F32(60.0)), r).astype(F32)
    t = F32(1000.0)
    s = ref.sanitise(r)
    assert (display_ref.luminance(s) < t).all()
    out, _ = ref.glare(r, ref.make(1.0, 1.0, t, 8))
    fin = np.isfinite(r).all(axis=-1)
    assert np.array_equal(out[fin].view(np.uint32), s[fin].view(np.uint32)) and np.array_equal(out[~fin].view(np.uint32), r[~fin].view(np.uint32))


def test_huge_inputs_produce_no_inf_or_nan():
    big = F32(2.0 ** 64)
    values = (np.finfo(F32).max, big, np.nextafter(big, F32(0)), np.nextafter(big, F32(np.inf)), F32(2.0 ** 100))
    for (nx, rows), (a, sp, t, L) in itertools.product(((1, 1), (2, 2), (7, 13), (64, 64)), ((1.0, 1.0, 0.0, 8), (1.0, 0.5, 1.0, 3), (0.3, 1.0, 3e38, 8))):
        for v in values:
            checker = np.indices((rows, nx)).sum(axis=0)[..., None] % 2 == 0
            for c in (np.full((rows, nx, 3), v, F32), np.where(checker, v, F32(1e-30)).astype(F32) * np.ones(3, F32)):
                out, info = ref.glare(c, ref.make(a, sp, t, L))
                assert np.isfinite(out).all() and (out >= 0).all() and out.max() <= big * F32(1.0001), (nx, rows, v)
                for x in info["d"] + info["u"]:
                    assert np.isfinite(x).all()


def test_the_ambiguous_share_of_the_glared_planes_stays_under_the_cap():
    """The GPU test compares out_rgb8 under {KEY, ACES, SRGB, BAYER8} outside display_ref's ambiguous mask, with display_ref's cap on its
    share: the planes it uses stay within that cap on the reference alone."""
    d = display_ref.make(0.18, auto=display_ref.KEY, curve=display_ref.ACES, transfer=display_ref.SRGB, dither=display_ref.BAYER8)
    for (nx, rows), (name, plane) in itertools.product(ref.FRAMES, ref.PLANES):
        out, _ = ref.glare(plane(nx, rows), ref.make(0.25, 0.5, 0.0, 3))
        _, info = display_ref.display(out, d)
        share = float(info["ambiguous"].mean())
        assert share <= display_ref.AMBIGUOUS_CAP, (nx, rows, name, share)
