"""The half buffers without a GPU: the new symbols and struct layouts against the C compiler, n_h against brute force, rt_accum_halves_check
through ctypes on each refusal, csrc/rt_halves_plan.h as a stand-alone program under AddressSanitizer + UBSan, the .npz round trip of
AccumHalves, and the designed half states of tests/halves_ref.py: that they have the properties they are built for, on the reference alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
import halves_ref as ref
import noise_tree_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rt_accum_track_halves", "rt_accum_read_halves", "rt_accum_denoise_halves", "rt_accum_halves_check", "rt_accum_export_halves",
               "rt_accum_import_halves"]


def test_symbols_and_struct_layouts_match_the_c_compiler(rt, tmp_path):
    f = rt._ffi
    lib = f.load_gpu_library()
    assert lib.rt_abi_version() == 11 == f.EXPECTED_ABI  # only symbols and two structs were added
    for n in NEW_SYMBOLS:
        assert n in f.GPU_SYMBOLS and hasattr(lib, n), n
    hf = [n for n, _ in f.RtAccumHalves._fields_]
    rf = [n for n, _ in f.RtResidual._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x.h"\n'
                   'int main(void){int (*a)(RtCtx*) = rt_accum_track_halves;\n'
                   'int (*b)(RtCtx*, uint32_t, float*, float*) = rt_accum_read_halves;\n'
                   'int (*c)(RtCtx*, const RtDenoise*, float*, uint8_t*, float*, RtResidual*) = rt_accum_denoise_halves;\n'
                   'int (*d)(const RtAccumHalves*) = rt_accum_halves_check;\n'
                   'int (*e)(RtCtx*, RtAccumHalves*) = rt_accum_export_halves;\n'
                   'int (*g)(RtCtx*, const RtAccumHalves*) = rt_accum_import_halves;\n'
                   'printf("%zu' + " %zu" * (len(hf) + 1 + len(rf)) + ' %d %.9g %u\\n", sizeof(RtAccumHalves), ' +
                   ", ".join("offsetof(RtAccumHalves, %s)" % n for n in hf) + ", sizeof(RtResidual), " +
                   ", ".join("offsetof(RtResidual, %s)" % n for n in rf) +
                   ', (a != 0) + (b != 0) + (c != 0) + (d != 0) + (e != 0) + (g != 0), (double)RT_DENOISE_HALVES_DEFAULT_STRENGTH, RT_ABI_VERSION);'
                   'return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", os.path.dirname(f.GPU_LIB_PATH),
                    "-l:librtow_mi355x.so", "-Wl,-rpath," + os.path.dirname(f.GPU_LIB_PATH), "-Wl,--allow-shlib-undefined"], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    H, R = f.RtAccumHalves, f.RtResidual
    want = [C.sizeof(H)] + [getattr(H, n).offset for n in hf] + [C.sizeof(R)] + [getattr(R, n).offset for n in rf] + [6]
    assert [int(x) for x in got[:len(want)]] == want and (C.sizeof(H), C.sizeof(R)) == (64, 32)
    assert np.float32(got[-2]) == np.float32(f.DENOISE_HALVES_DEFAULT_STRENGTH) and int(got[-1]) == 11
    assert hf == ["nx", "rows", "first_sample", "done", "reserved", "frame_id", "sum", "moments"]
    assert rf == ["mean_luminance", "residual_rms", "residual_noise", "reserved"]


def test_half_counts_against_brute_force(rt):
    for first in (0, 1, 2 ** 32 - 2):
        for n in range(10):
            if first + n > 2 ** 32 - 1:
                continue
            h = rt.AccumHalves(1, 1, first_sample=first, done=n)
            for k in range(2):
                assert ref.n_h(first, n, k) == ref.n_h_brute(first, n, k) == int(h.counts()[k]), (first, n, k)
    assert (ref.n_h(0, 2 ** 32 - 1, 0), ref.n_h(0, 2 ** 32 - 1, 1)) == (2 ** 31, 2 ** 31 - 1)
    h = rt.AccumHalves(1, 1, first_sample=0, done=2 ** 32 - 1)
    assert [int(x) for x in h.counts()] == [2 ** 31, 2 ** 31 - 1]
    cnt = np.array([[0, 1, 2, 3, 8]], np.uint32)
    for first in (4, 7):
        n0, n1 = rt.AccumHalves(5, 1, first_sample=first).counts(cnt)
        assert n0.tolist() == [[ref.n_h_brute(first, int(n), 0) for n in cnt[0]]] and (n0 + n1 == cnt).all()
        assert ref.n_h(first, cnt, 1).tolist() == n1.tolist()


def test_halves_check_of_the_library_on_each_refusal(rt):
    lib = rt._ffi.load_gpu_library()
    inv = -rt._ffi.ERR_INVALID
    assert lib.rt_accum_halves_check(None) == inv
    h = rt.AccumHalves(5, 3, first_sample=3, done=7, frame_id=99)
    assert h.check() and lib.rt_accum_halves_check(C.byref(h.as_struct())) == 0
    for k in range(2):
        hs = h.as_struct()
        hs.reserved[k] = 1
        assert lib.rt_accum_halves_check(C.byref(hs)) == inv
        hs = h.as_struct()
        hs.sum[k] = None
        assert lib.rt_accum_halves_check(C.byref(hs)) == inv
        hs = h.as_struct()
        hs.moments[k] = None
        assert lib.rt_accum_halves_check(C.byref(hs)) == inv
    h.first_sample, h.done = 2 ** 32 - 1 - 7, 7
    assert h.check()
    h.first_sample += 1
    assert not h.check()
    h.first_sample = 3
    h.sum[0, 0, 0, 0], h.moments[1, 0, 0, 1] = np.nan, np.inf  # values are not judged
    assert h.check()
    hs = h.as_struct()
    for fn in (lib.rt_accum_export_halves, lib.rt_accum_import_halves):  # the entry points refuse without a context, and need no device to say so
        assert fn(None, C.byref(hs)) == inv
    assert lib.rt_accum_track_halves(None) == inv and lib.rt_accum_read_halves(None, 0, None, None) == inv
    assert lib.rt_accum_denoise_halves(None, None, None, None, None, None) == inv
    with pytest.raises(ValueError):
        rt.AccumHalves(4, 2, sum=np.zeros((2, 2, 4, 2), np.float32))


def test_npz_round_trip_is_bit_for_bit(rt, tmp_path):
    rng = np.random.default_rng(5)
    h = rt.AccumHalves(7, 3, first_sample=4, done=2 ** 32 - 5, frame_id=2 ** 64 - 3, sum=rng.random((2, 3, 7, 3), dtype=np.float32),
                       moments=rng.random((2, 3, 7, 2)))
    h.sum.view(np.uint32)[1, 0, 0] = [0x7FC01234, 0x80000000, 0xFF800000]
    h.moments.view(np.uint64)[0, 2, 6] = [0x7FF8DEADBEEF0001, 0xFFF0000000000000]
    path = str(tmp_path / "halves.npz")
    h.save(path)
    assert os.listdir(tmp_path) == ["halves.npz"]
    t = rt.AccumHalves.load(path)
    assert all(getattr(t, k) == getattr(h, k) for k in ("nx", "rows", "first_sample", "done", "frame_id"))
    assert np.array_equal(t.sum.view(np.uint32), h.sum.view(np.uint32)) and np.array_equal(t.moments.view(np.uint64), h.moments.view(np.uint64))
    assert t.check()


def test_halves_plan_header_under_asan_ubsan(tmp_path):
    """csrc/rt_halves_plan.h compiled into tests/halves_plan_main.cpp with AddressSanitizer + UBSan: every section made its checks, none
    failed and no sanitizer reported."""
    exe = str(tmp_path / "halves_plan_san")
    c = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-Wall", "-Wextra",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray_tracing_in_one_weekend_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "halves_plan_main.cpp")], capture_output=True, text=True, timeout=600)
    if c.returncode != 0 and "sanitize" in c.stderr + c.stdout and "cannot find" in c.stderr + c.stdout:
        pytest.skip("sanitizer runtime not available")
    assert c.returncode == 0, c.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l[0] for l in lines] == ["counts", "check", "layout", "ok"]
    assert all(int(l[1]) > 0 for l in lines[:-1])


def test_parity_split_of_the_reference_on_hand_made_samples():
    """Values chosen so that a sum in another order, or in double precision, would differ: 2^24, then 1, 1, 1, 1."""
    vals = [16777216.0, 1.0, 1.0, 1.0, 1.0, 1.0, 3.0]
    frames = [np.full((1, 2, 3), v, np.float32) for v in vals]
    for first in (0, 7):
        halves = ref.split(frames, first)
        for h in range(2):
            mine = [v for k, v in enumerate(vals) if (first + k) & 1 == h]
            want = np.float32(0)
            for v in mine:
                want = np.float32(want + np.float32(v))
            assert halves[h][0][0, 0, 0] == want and halves[h][1][0, 0] == sum(mine)  # (luminance of a grey sample: 0.2126 + 0.7152 + 0.0722 = 1 within rounding)
        big = 0 if first == 0 else 1  # the half that holds 2^24 swallows its ones one by one: 2^24 + 3 only, rounded to even
        assert halves[big][0][0, 0, 0] == 16777220.0 and halves[1 - big][0][0, 0, 0] == 3.0
    counts = np.array([[3, 6]], np.uint32)
    halves = ref.split(frames, 7, counts)  # pixel 0 holds samples 7, 8, 9; pixel 1 holds 7 .. 12
    assert halves[1][0][0, :, 0].tolist() == [16777216.0, 16777216.0] and halves[0][0][0, :, 0].tolist() == [1.0, 3.0]
    assert halves[1][1][0].tolist() == [16777217.0, 16777218.0]  # (S1 in f64 keeps the ones: luminance of a grey sample is its value here)


def test_designed_half_states_have_the_properties_they_are_built_for():
    # the kernel case: every weight class holds >= 10 % of the pairs in both directions; NaN and +inf in half 0 only; a block with v = 0
    halves = ref.kernel_halves(37, 21)
    r = ref.cross_filter(halves, 0, 16, 5, 1, denoise_ref.KERNEL_CASE_STRENGTH)
    for shares in r["shares"]:
        assert min(shares) >= 0.10, shares
    (c0, y0, v0), (c1, y1, v1) = r["inputs"]
    assert np.isnan(y0).sum() == 1 and np.isinf(y0).sum() == 1 and np.isfinite(y1).all() and np.isfinite(v1).all() and np.isfinite(c1).all()
    assert (v0 == 0).sum() >= 16 and (v1 == 0).sum() >= 16
    bad = ~np.isfinite(c0).all(-1)
    # A non-finite colour in ONE half: the other half's guide is finite there, so f_0 spreads it over the window (the header says so); f_1,
    # guided by the half that holds it, keeps it out.  It reaches no pixel further than R away.
    spread = ~np.isfinite(r["out"]).all(-1)
    assert bad.sum() == 2 and spread[bad].all() and np.isfinite(r["f"][1]).all() and spread.sum() > 2
    ys, xs = np.nonzero(bad)
    near = np.zeros_like(bad)
    for y, x in zip(ys, xs):
        near[max(y - 5, 0):y + 6, max(x - 5, 0):x + 6] = True
    assert not spread[~near].any()
    assert np.isnan(r["residual"][0]) and np.isnan(r["residual"][1])
    # the plain synthetic halves: finite figures, residual below the mean
    p = ref.cross_filter(ref.plain_halves(37, 21), 0, 16, 5, 1, 0.45)
    assert all(np.isfinite(p["residual"])) and 0 < p["residual"][2] < 1 and min(min(s) for s in p["shares"]) >= 0.10
    # the adaptive state: pixels with n_p in {0, 1, 2, 3} beside done = 8, and what the halves make of them for both parities of first_sample
    cnt, conv = ref.adaptive_counts(37, 21)
    assert set(np.unique(cnt)) == {0, 1, 2, 3, 8} and ((cnt == 8) == (conv == 0)).all()
    for first in (4, 7):
        n0, n1 = ref.n_h(first, cnt, 0), ref.n_h(first, cnt, 1)
        assert {(int(a), int(b)) for a, b in zip(n0.ravel(), n1.ravel())} == \
            ({(0, 0), (1, 0), (1, 1), (2, 1), (4, 4)} if first == 4 else {(0, 0), (0, 1), (1, 1), (1, 2), (4, 4)})
        a = ref.cross_filter(ref.plain_halves(37, 21, nh=4), first, cnt, 5, 1, 0.45)
        assert min(min(s) for s in a["shares"]) >= 0.05  # (the designed pixels are sparse and the active ones hold 4 samples per half: every weight class is there)
        none = (n0 == 0) | (n1 == 0)
        assert (np.isnan(a["err"]) == none).all() and np.isfinite(a["out"]).all()
        one = (n1 == 0) if first == 4 else (n0 == 0) & (n1 != 0)  # (a pixel without any sample: f_0, its zeros)
        assert np.array_equal(a["out"][one], a["f"][0 if first == 4 else 1][one])
    # 257 x 256: more than 256 partial sums, the extremes of e behind pixel 65 536, and a final sum that needs its tail
    e = ref.cross_filter(ref.extremes_halves(), 0, 16, 1, 0, 0.45)
    err = e["err"].reshape(-1)
    assert -(-err.size // 256) > 256 and int(np.argmax(err)) > 65536 and np.isfinite(err).all()
    assert err.max() > 1e3 * np.median(err)
    lum, e64 = ref.lum32(e["out"]).astype(np.float64).reshape(-1), err.astype(np.float64)
    assert noise_tree_ref.figures(lum, e64, 2, tail=False) != e["residual"]
