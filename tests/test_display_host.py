"""The display transform without a GPU: the new symbols and struct layouts against the C compiler, B, the identity configuration of
tests/display_ref.py against the reference quantisation on every step boundary, the histogram's bin edges, rt_display_check through ctypes
on each refusal, csrc/rt_display_plan.h as a stand-alone program under AddressSanitizer + UBSan, the share of ambiguous sRGB values on the
planes the GPU test uses — on the reference alone —, and the PFM round trip."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
import designed_states
import display_ref as ref
import noise_tree_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_symbols_and_struct_layouts_match_the_c_compiler(rt, tmp_path):
    f = rt._ffi
    lib = f.load_gpu_library()
    for n in ("rt_set_display", "rt_display_info", "rt_display_check", "rt_debug_display"):
        assert n in f.GPU_SYMBOLS and hasattr(lib, n), n
    df, inf_ = [n for n, _ in f.RtDisplay._fields_], [n for n, _ in f.RtDisplayInfo._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x_debug.h"\n'
                   'int main(void){int (*a)(RtCtx*, const RtDisplay*) = rt_set_display;\n'
                   'int (*b)(RtCtx*, RtDisplayInfo*) = rt_display_info;\n'
                   'int (*c)(const RtDisplay*) = rt_display_check;\n'
                   'int (*d)(RtCtx*, uint32_t, uint32_t, const float*, const RtDisplay*, uint8_t*, RtDisplayInfo*) = rt_debug_display;\n'
                   'printf("%zu' + " %zu" * (len(df) + 1 + len(inf_)) + ' %d %d %d %d %d %.17g %u\\n", sizeof(RtDisplay), ' +
                   ", ".join("offsetof(RtDisplay, %s)" % n for n in df) + ", sizeof(RtDisplayInfo), " +
                   ", ".join("offsetof(RtDisplayInfo, %s)" % n for n in inf_) +
                   ', (a != 0) + (b != 0) + (c != 0) + (d != 0), (int)RT_EXPOSURE_PERCENTILE, (int)RT_TONE_ACES, (int)RT_TRANSFER_SRGB,'
                   ' (int)RT_DITHER_BAYER8, (double)RT_DISPLAY_SRGB_EPS, RT_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", os.path.dirname(f.GPU_LIB_PATH),
                    "-l:librtow_mi355x.so", "-Wl,-rpath," + os.path.dirname(f.GPU_LIB_PATH), "-Wl,--allow-shlib-undefined"], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    D, I = f.RtDisplay, f.RtDisplayInfo
    want = [C.sizeof(D)] + [getattr(D, n).offset for n in df] + [C.sizeof(I)] + [getattr(I, n).offset for n in inf_]
    assert [int(x) for x in got[:len(want)]] == want and (C.sizeof(D), C.sizeof(I)) == (32, 40)
    assert [int(x) for x in got[len(want):len(want) + 5]] == [4, f.EXPOSURE_PERCENTILE, f.TONE_ACES, f.TRANSFER_SRGB, f.DITHER_BAYER8]
    assert float(got[-2]) == f.DISPLAY_SRGB_EPS == ref.EPS and int(got[-1]) == 11
    assert df == ["exposure_mode", "exposure_value", "percentile", "curve", "white", "transfer", "dither", "reserved"]
    assert inf_ == ["exposure", "percentile_luminance", "log_average", "n_lit", "n_non_finite", "n_saturated"]
    assert (ref.MANUAL, ref.KEY, ref.PERCENTILE) == (f.EXPOSURE_MANUAL, f.EXPOSURE_KEY, f.EXPOSURE_PERCENTILE)
    assert (ref.CLAMP, ref.REINHARD, ref.ACES, ref.GAMMA2, ref.SRGB, ref.NONE, ref.BAYER8) == (f.TONE_CLAMP, f.TONE_REINHARD, f.TONE_ACES, f.TRANSFER_GAMMA2,
                                                                                             f.TRANSFER_SRGB, f.DITHER_NONE, f.DITHER_BAYER8)


def test_bayer_index_is_the_permutation_of_the_header():
    x, y = np.meshgrid(np.arange(8), np.arange(8))
    b = ref.bayer(x, y)
    assert sorted(b.reshape(-1).tolist()) == list(range(64))
    assert b[0].tolist() == [0, 32, 8, 40, 2, 34, 10, 42]
    assert b[:2, :2].tolist() == [[0, 32], [48, 16]]  # the 2 x 2 matrix [[0, 2], [3, 1]] in the leading bits
    # an ordered dither: over one tile a constant y reaches the upper of its two levels in the share of the tile its fraction asks for
    for level, frac in ((17, 0.0), (17, 0.25), (200, 0.5), (3, 63.0 / 64.0)):
        img = np.full((8, 8, 3), ((level + frac) / 255.0) ** 2, F32)
        u, _ = ref.display(img, ref.make(dither=ref.BAYER8))
        assert set(np.unique(u)) <= {level, level + 1} and abs(int((u[..., 0] == level + 1).sum()) - round(64 * frac)) <= 1, (level, frac)


def test_identity_configuration_is_the_reference_quantisation():
    """{MANUAL, 1, CLAMP, GAMMA2, NONE} against denoise_ref.finalize_rgb8 on the quantisation bits: either side of every step, +-0, the
    smallest denormal, FLT_MIN, 1 -+ ulp, FLT_MAX, the infinities, -1 and a NaN."""
    vals = designed_states.f32_of_bits(designed_states.quantisation_bits())
    for rows in (1, 3):
        img = np.repeat(np.resize(vals, rows * 175 * 3).reshape(rows, 175, 3), 1, axis=0)
        u, info = ref.display(img, ref.make())
        assert np.array_equal(u, denoise_ref.finalize_rgb8(img))
        assert info["exposure"] == 1 and info["n_saturated"] == int((u == 255).sum()) and info["ambiguous"] is None
        assert info["n_non_finite"] == int((~np.isfinite(img)).any(axis=-1).sum()) > 0
    px = ref.designed_pixels()
    assert np.array_equal(ref.display(px[None], ref.make())[0], denoise_ref.finalize_rgb8(px[None]))
    bad = ~np.isfinite(px)
    assert {int(b.sum()) for b in bad} == {0, 1, 2, 3} and (px < 0).any() and np.isnan(px).any() and np.isposinf(px).any() and np.isneginf(px).any()


def test_the_bin_edges():
    f = designed_states.f32_of_bits
    for bits, want in ((0x00000001, 0), (0x007FFFFF, 7), (0x00800000, 8), (0x3F7FFFFF, 1015), (0x3F800000, 1016), (0x3F87FFFF, 1016), (0x3F880000, 1016),
                       (0x3F8FFFFF, 1016), (0x3F900000, 1017), (0x40000000, 1024), (0x7F7FFFFF, 2039)):  # the smallest denormal, FLT_MIN, 1 - ulp, 1, FLT_MAX
        hist, n_lit = ref.histogram_y(f([bits]))
        assert n_lit == 1 and hist[want] == 1 and hist.sum() == 1, (hex(bits), want, np.flatnonzero(hist))
    for bits in (0x00000000, 0x80000000, 0x80000001, 0xBF800000, 0x7F800000, 0xFF800000, 0x7FC01234):  # +-0, negatives, the infinities, a NaN: not lit
        hist, n_lit = ref.histogram_y(f([bits]))
        assert n_lit == 0 and hist.sum() == 0, hex(bits)
    # the luminance, not a channel, decides: a green of 1 / 0.7152f lands in the bin of 1 (or the one below, by the product's rounding)
    img = np.array([[[0, F32(1) / F32(0.7152), 0]]], F32)
    hist, n_lit = ref.histogram(img)
    assert n_lit == 1 and hist[int(np.array([ref.luminance(img)[0, 0]]).view(np.uint32)[0]) >> 20] == 1 and hist[1015:1017].sum() == 1
    assert ref.bin_mid(1016) == F32(1.0625) and ref.bin_mid(0) == designed_states.f32_of_bits([0x00080000])[0] and np.isfinite(ref.bin_mid(2039))
    assert ref.rank_of(1.0, 66000) == 66000 and ref.rank_of(2.0 ** -20, 66000) == 1 and ref.rank_of(0.5, 3) == 2 and ref.rank_of(0.99, 100) == 100


def test_statistics_of_the_reference_on_hand_made_images():
    # a constant image: every percentile is the bin of its luminance; the key exposure maps the luminance onto the key
    img = np.full((5, 7, 3), 0.25, F32)
    Y = ref.luminance(img)[0, 0]
    for q in (2.0 ** -20, 0.5, 1.0):
        s = ref.statistics(img, ref.make(0.5, auto=ref.PERCENTILE, percentile=q))
        assert s["n_lit"] == 35 and s["percentile_luminance"] == ref.bin_mid(int(np.array([Y]).view(np.uint32)[0]) >> 20)
        assert s["exposure"] == F32(np.float64(F32(0.5)) / np.float64(s["percentile_luminance"]))
    s = ref.statistics(img, ref.make(0.18, auto=ref.KEY))
    assert abs(s["log_average"] / float(Y) - 1) < 1e-14 and abs(float(s["exposure"]) * float(Y) / 0.18 - 1) < 1e-6
    # nothing lit: e = 1
    for mode in (ref.KEY, ref.PERCENTILE):
        s = ref.statistics(np.zeros((2, 2, 3), F32), ref.make(0.18, auto=mode))
        assert s["n_lit"] == 0 and s["exposure"] == 1 and s["percentile_luminance"] == 0 and s["log_average"] == 0
    # the tree reaches the second trip of the final loop on the large frame: dropping the tail changes the sum
    big = ref.statistics_plane(300, 220)
    y = ref.luminance(big).reshape(-1)
    lit = np.isfinite(y) & (y > 0)
    logs = np.where(lit, np.log(np.where(lit, y, 1).astype(np.float64)), 0.0)
    assert noise_tree_ref.tree_sum(logs) != noise_tree_ref.tree_sum(logs, tail=False) and (~lit).sum() > 1000 and lit[65536 + 100] and lit[65536 + 300]
    assert abs(noise_tree_ref.tree_sum(logs) - float(np.sum(logs))) < 1e-6


def test_display_check_refuses_every_invalid_field(rt):
    assert not rt.display_check(None)
    good = dict(exposure=0.5, auto="percentile", percentile=0.99, curve="reinhard", white=4.0, transfer="srgb", dither="bayer8")
    assert rt.display_check(rt.make_display(**good)) and rt.display_check(rt.make_display())
    for field, top in (("exposure_mode", 2), ("curve", 2), ("transfer", 1), ("dither", 1)):
        d = rt.make_display(**good)
        setattr(d, field, top + 1)
        assert not rt.display_check(d), field
        setattr(d, field, 0xFFFFFFFF)
        assert not rt.display_check(d), field
    d = rt.make_display(**good)
    d.reserved = 1
    assert not rt.display_check(d)
    for mode in ("manual", "key", "percentile"):
        for v in (0.0, -1.0, np.inf, -np.inf, np.nan):
            assert not rt.display_check(rt.make_display(**dict(good, auto=None if mode == "manual" else mode, exposure=v))), (mode, v)
    for q in (0.0, -0.5, float(np.nextafter(F32(1), F32(2))), np.inf, np.nan):
        assert not rt.display_check(rt.make_display(**dict(good, percentile=q))), q
        assert rt.display_check(rt.make_display(**dict(good, percentile=q, auto="key")))  # ignored outside PERCENTILE
    assert rt.display_check(rt.make_display(**dict(good, percentile=1.0))) and rt.display_check(rt.make_display(**dict(good, percentile=2.0 ** -20)))
    for w in (0.0, -1.0, -np.inf, np.nan):
        assert not rt.display_check(rt.make_display(**dict(good, white=w))), w
        assert rt.display_check(rt.make_display(**dict(good, white=w, curve="aces")))  # ignored outside REINHARD
    assert rt.display_check(rt.make_display(**dict(good, white=np.inf)))


def test_display_plan_header_under_asan_ubsan(tmp_path):
    """csrc/rt_display_plan.h compiled into tests/display_plan_main.cpp with AddressSanitizer + UBSan: every section made its checks, none
    failed and no sanitizer reported."""
    exe = str(tmp_path / "display_plan_san")
    c = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-Wall", "-Wextra",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray_tracing_in_one_weekend_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "display_plan_main.cpp")], capture_output=True, text=True, timeout=600)
    if c.returncode != 0 and "sanitize" in c.stderr + c.stdout and "cannot find" in c.stderr + c.stdout:
        pytest.skip("sanitizer runtime not available")
    assert c.returncode == 0, c.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l[0] for l in lines] == ["check", "bayer", "rank", "bins", "exposure", "ok"]
    assert all(int(l[1]) > 0 for l in lines[:-1])


def test_the_ambiguous_share_of_the_reference_stays_under_the_cap():
    """Under the sRGB transfer a value is ambiguous where y (1 - EPS) and y (1 + EPS) quantise to different levels.  On the planes of the
    GPU test the share stays far below the cap (on uniform y it is about 2 EPS x 255: 5e-4), the two levels are neighbours, and the
    plane that sits 8 EPS on either side of every boundary holds none."""
    for (nx, rows), curve, dither in itertools.product(ref.FRAMES, (ref.CLAMP, ref.REINHARD, ref.ACES), (ref.NONE, ref.BAYER8)):
        for plane, e in ((ref.designed_plane(nx, rows), 1.0), (ref.log_uniform_plane(nx, rows), 0.37)):
            u, info = ref.display(plane, ref.make(e, curve=curve, white=3.0, transfer=ref.SRGB, dither=dither))
            a = info["ambiguous"]
            share = a.mean()
            assert share <= ref.AMBIGUOUS_CAP, (nx, rows, curve, dither, share)
            assert (info["level_hi"].astype(int) - info["level_lo"])[a].max(initial=1) == 1 and np.array_equal(info["level_lo"][~a], u[~a])
    y = np.random.default_rng(3).random(1 << 20)
    lo, hi = np.floor(y * (1 - ref.EPS) * 255.99), np.floor(y * (1 + ref.EPS) * 255.99)
    assert 1e-4 < (lo != hi).mean() < 1e-3
    t = ref.srgb_boundary_values()
    img = np.repeat(t.reshape(1, -1, 1), 3, axis=2)
    u, info = ref.display(img, ref.make(transfer=ref.SRGB))
    assert not info["ambiguous"].any()
    k = np.arange(1, 256)
    assert np.array_equal(u[0, :255, 0], k - 1) and np.array_equal(u[0, 255:, 0], k)  # below the boundary the level before it, above it the level


def test_pfm_round_trip(rt, tmp_path):
    from ray_tracing_in_one_weekend_amd import images
    img = np.random.default_rng(1).normal(size=(5, 7, 3)).astype(F32) * F32(1e3)
    img.view(np.uint32)[0, 0] = [0x7FC01234, 0x7F800000, 0xFF800000]
    img[4, 6] = [0.0, -0.0, np.finfo(F32).max]
    path = str(tmp_path / "frame.pfm")
    images.write_pfm(path, img)
    raw = open(path, "rb").read()
    assert raw.startswith(b"PF\n7 5\n-1.0\n") and len(raw) == len(b"PF\n7 5\n-1.0\n") + 5 * 7 * 12
    assert raw[-12:] == img[4, 6].tobytes()  # row 0 of the image, the bottom one, comes first: the last bytes are the top row's last pixel
    back = images.read_pfm(path)
    assert back.dtype == F32 and np.array_equal(back.view(np.uint32), img.view(np.uint32))
    big = str(tmp_path / "big_endian.pfm")
    with open(big, "wb") as f:
        f.write(b"PF\n7 5\n1.0\n" + img.astype(">f4").tobytes())
    assert np.array_equal(images.read_pfm(big).view(np.uint32)[1:], img.view(np.uint32)[1:])
