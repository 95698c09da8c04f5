"""The sample buckets without a GPU: the new symbols and struct layouts against the C compiler, n_b against brute force,
rt_accum_buckets_check through ctypes on each refusal, csrc/rt_buckets_plan.h as a stand-alone program under AddressSanitizer + UBSan, the
.npz round trip of AccumBuckets, the reference of tests/robust_ref.py on hand-made bucket means with expected values written out, the
designed states the GPU test imports, and what the estimator is and is not on two synthetic frames."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import noise_tree_ref
import robust_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ["rt_accum_track_buckets", "rt_accum_read_robust", "rt_accum_denoise_robust", "rt_accum_buckets_check", "rt_accum_export_buckets",
               "rt_accum_import_buckets"]


def test_symbols_and_struct_layouts_match_the_c_compiler(rt, tmp_path):
    f = rt._ffi
    lib = f.load_gpu_library()
    assert lib.rt_abi_version() == 11 == f.EXPECTED_ABI  # only symbols and three structs were added
    for n in NEW_SYMBOLS:
        assert n in f.GPU_SYMBOLS and hasattr(lib, n), n
    structs = [("RtAccumBuckets", f.RtAccumBuckets), ("RtRobust", f.RtRobust), ("RtRobustInfo", f.RtRobustInfo)]
    probes = []
    for name, S in structs:
        probes += ["sizeof(%s)" % name] + ["offsetof(%s, %s)" % (name, n) for n, _ in S._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x.h"\n'
                   'int main(void){int (*a)(RtCtx*, uint32_t) = rt_accum_track_buckets;\n'
                   'int (*b)(RtCtx*, const RtRobust*, float*, uint8_t*, uint8_t*, RtRobustInfo*) = rt_accum_read_robust;\n'
                   'int (*c)(RtCtx*, const RtRobust*, const RtDenoise*, float*, uint8_t*) = rt_accum_denoise_robust;\n'
                   'int (*d)(const RtAccumBuckets*) = rt_accum_buckets_check;\n'
                   'int (*e)(RtCtx*, RtAccumBuckets*) = rt_accum_export_buckets;\n'
                   'int (*g)(RtCtx*, const RtAccumBuckets*) = rt_accum_import_buckets;\n'
                   'printf("' + "%zu " * len(probes) + '%d %u %u %u %u %u\\n", ' + ", ".join(probes) +
                   ', (a != 0) + (b != 0) + (c != 0) + (d != 0) + (e != 0) + (g != 0), RT_BUCKETS_MAX, RT_ROBUST_GINI, RT_ROBUST_MEDIAN, RT_ROBUST_TRIM, '
                   'RT_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", os.path.dirname(f.GPU_LIB_PATH),
                    "-l:librtow_mi355x.so", "-Wl,-rpath," + os.path.dirname(f.GPU_LIB_PATH), "-Wl,--allow-shlib-undefined"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, S in structs:
        want += [C.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_]
    assert got == want + [6, f.BUCKETS_MAX, f.ROBUST_GINI, f.ROBUST_MEDIAN, f.ROBUST_TRIM, 11]
    assert [C.sizeof(S) for _, S in structs] == [160, 16, 40] and f.BUCKETS_MAX == 16 == ref.BUCKETS_MAX
    assert [n for n, _ in f.RtAccumBuckets._fields_] == ["nx", "rows", "first_sample", "done", "M", "reserved", "frame_id", "sum"]
    assert [n for n, _ in f.RtRobust._fields_] == ["mode", "trim", "reserved"]
    assert [n for n, _ in f.RtRobustInfo._fields_] == ["mean_luminance_plain", "mean_luminance_robust", "energy_removed", "trimmed_fraction", "nonfinite_dropped"]
    assert (ref.GINI, ref.MEDIAN, ref.TRIM) == (f.ROBUST_GINI, f.ROBUST_MEDIAN, f.ROBUST_TRIM)
    for name in ("AccumBuckets", "RtAccumBuckets", "RtRobust", "RtRobustInfo"):
        assert name in rt.__all__ and hasattr(rt, name)


def test_bucket_counts_against_brute_force(rt):
    for M in (3, 5, 16):
        for n in (0, 1, M - 1, M, M + 1, 2 * M + 3):
            for first in (0, 1, M - 1, 2 ** 32 - 1 - n):
                h = rt.AccumBuckets(1, 1, M, first_sample=first, done=n)
                mine = [ref.n_b(first, n, M, b) for b in range(M)]
                assert mine == [ref.n_b_brute(first, n, M, b) for b in range(M)] == [int(x) for x in h.counts()], (M, n, first)
                assert sum(mine) == n
    assert sum(ref.n_b(0, 2 ** 32 - 1, 5, b) for b in range(5)) == 2 ** 32 - 1
    cnt = np.array([[0, 1, 4, 5, 6, 13]], np.uint32)
    for first in (0, 7):
        got = rt.AccumBuckets(6, 1, 5, first_sample=first).counts(cnt)
        assert got.tolist() == [[[ref.n_b_brute(first, int(n), 5, b) for n in cnt[0]]] for b in range(5)] and (got.sum(0) == cnt).all()
        assert [ref.n_b(first, cnt, 5, b).tolist() for b in range(5)] == got.tolist()


def test_buckets_check_of_the_library_on_each_refusal(rt):
    lib = rt._ffi.load_gpu_library()
    inv = -rt._ffi.ERR_INVALID
    assert lib.rt_accum_buckets_check(None) == inv
    h = rt.AccumBuckets(5, 3, 5, first_sample=3, done=7, frame_id=99)
    assert h.check() and lib.rt_accum_buckets_check(C.byref(h.as_struct())) == 0
    bs = h.as_struct()
    bs.reserved = 1
    assert lib.rt_accum_buckets_check(C.byref(bs)) == inv
    for k in range(5):
        bs = h.as_struct()
        bs.sum[k] = None
        assert lib.rt_accum_buckets_check(C.byref(bs)) == inv
    for M in (0, 2, 17):
        bs = h.as_struct()
        bs.M = M
        assert lib.rt_accum_buckets_check(C.byref(bs)) == inv
        assert not rt.AccumBuckets(5, 3, M).check()
    bs = h.as_struct()
    bs.M = 3  # the pointers past M are not looked at
    assert lib.rt_accum_buckets_check(C.byref(bs)) == 0
    assert rt.AccumBuckets(2, 2, 3).check() and rt.AccumBuckets(2, 2, 16).check()
    h.first_sample, h.done = 2 ** 32 - 1 - 7, 7
    assert h.check()
    h.first_sample += 1
    assert not h.check()
    h.first_sample = 3
    h.sum[0, 0, 0, 0], h.sum[4, 2, 4, 2] = np.nan, np.inf  # values are not judged
    assert h.check()
    bs = h.as_struct()
    for fn in (lib.rt_accum_export_buckets, lib.rt_accum_import_buckets):  # the entry points refuse without a context, and need no device to say so
        assert fn(None, C.byref(bs)) == inv
    assert lib.rt_accum_track_buckets(None, 5) == inv and lib.rt_accum_read_robust(None, None, None, None, None, None) == inv
    assert lib.rt_accum_denoise_robust(None, None, None, None, None) == inv
    with pytest.raises(ValueError):
        rt.AccumBuckets(4, 2, 5, sum=np.zeros((4, 2, 4, 3), np.float32))


def test_npz_round_trip_is_bit_for_bit(rt, tmp_path):
    rng = np.random.default_rng(5)
    h = rt.AccumBuckets(7, 3, 9, first_sample=4, done=2 ** 32 - 5, frame_id=2 ** 64 - 3, sum=rng.random((9, 3, 7, 3), dtype=np.float32))
    h.sum.view(np.uint32)[8, 0, 0] = [0x7FC01234, 0x80000000, 0xFF800000]
    path = str(tmp_path / "buckets.npz")
    h.save(path)
    assert os.listdir(tmp_path) == ["buckets.npz"]
    t = rt.AccumBuckets.load(path)
    assert all(getattr(t, k) == getattr(h, k) for k in ("nx", "rows", "first_sample", "done", "M", "frame_id"))
    assert np.array_equal(t.sum.view(np.uint32), h.sum.view(np.uint32)) and t.check()


def test_buckets_plan_header_under_asan_ubsan(tmp_path):
    """csrc/rt_buckets_plan.h compiled into tests/buckets_plan_main.cpp with AddressSanitizer + UBSan: every section made its checks, none
    failed and no sanitizer reported."""
    exe = str(tmp_path / "buckets_plan_san")
    c = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-Wall", "-Wextra",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray_tracing_in_one_weekend_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "buckets_plan_main.cpp")], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l[0] for l in lines] == ["counts", "check", "layout", "ok"]
    assert all(int(l[1]) > 0 for l in lines[:-1])


def test_split_of_the_reference_on_hand_made_samples():
    """Values chosen so that a sum in another order, or in double precision, would differ: 2^24, then ones."""
    vals = [16777216.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 3.0]
    frames = [np.full((1, 2, 3), v, F32) for v in vals]
    for first in (0, 7):
        got = ref.split(frames, first, 3)
        for b in range(3):
            want = F32(0)
            for k, v in enumerate(vals):
                if (first + k) % 3 == b:
                    want = F32(want + F32(v))
            assert got[b, 0, 0, 0] == want, (first, b)
        big = first % 3  # the bucket that holds 2^24 swallows its ones one by one
        assert got[big, 0, 0, 0] == 16777216.0 and sorted(got[:, 0, 0, 0].tolist()) == [2.0, 5.0, 16777216.0]
    got = ref.split(frames, 7, 3, np.array([[2, 5]], np.uint32))  # pixel 0 holds samples 7, 8; pixel 1 holds 7 .. 11
    assert got[:, 0, 0, 0].tolist() == [0.0, 16777216.0, 1.0] and got[:, 0, 1, 0].tolist() == [1.0, 16777216.0, 2.0]


def _read(means, mode=ref.GINI, trim=0):
    out, t, dropped = ref.means_readout(means, mode, trim)
    return float(out), t, dropped


def test_reference_on_hand_made_bucket_means():
    # equal means: Gn = 0, the mean of means
    assert _read([2.0] * 5) == (2.0, 0, 0)
    # one huge mean among five: s = 1004, w = 1 + 2 + 3 + 4 + 5000 = 5010, G = 10020 / 5020 - 1.2 = 0.796.., Gn = 0.995.., h = 2.48..: t = 2, the median
    assert _read([1.0, 1.0, 1000.0, 1.0, 1.0]) == (1.0, 2, 0)
    # milder: means 1 1 1 1 3: s = 7, w = 25, G = 50 / 35 - 1.2 = 0.2285.., Gn = 0.2857.., h = 0.714..: t = 0, the mean 7 / 5
    assert _read([1.0, 1.0, 3.0, 1.0, 1.0]) == (float(F32(7.0) / F32(5.0)), 0, 0)
    # means 1 1 1 1 6: s = 10, w = 40, G = 80 / 50 - 1.2 = 0.4, Gn = 0.5, h = 1.25: t = 1, (1 + 1 + 1) / 3
    assert _read([6.0, 1.0, 1.0, 1.0, 1.0]) == (1.0, 1, 0)
    # a NaN, a +inf and a -inf are dropped and counted; K = 2: x = 1, 2, s = 3, w = 5, G = 10 / 6 - 1.5 = 0.1666.., Gn = 0.333.., h = 0.333..: t = 0
    assert _read([np.nan, 2.0, np.inf, 1.0, -np.inf]) == (1.5, 0, 3)
    assert _read([np.nan, 2.0, np.inf, 1.0, -np.inf], ref.MEDIAN) == (1.5, 0, 3)  # (K - 1) / 2 = 0
    # all non-finite: NaN out, t = 0
    out, t, dropped = _read([np.nan, np.inf, -np.inf])
    assert out != out and (t, dropped) == (0, 3)
    # s <= 0: t = 0 whatever the spread; -0.0 alone gives +0 (every sum starts from +0)
    assert _read([-1000.0, 1.0, 1.0, 1.0, 1.0]) == (float(F32(-996.0) / F32(5.0)), 0, 0)
    assert _read([0.0] * 5) == (0.0, 0, 0)
    out, t, _ = ref.means_readout([-0.0] * 3)
    assert (t, out.view(np.uint32)) == (0, 0)
    out, t, _ = ref.means_readout([-0.0, 0.0, -0.0, 0.0], ref.MEDIAN)
    assert (t, out.view(np.uint32)) == (1, 0)
    # ties: 1 1 1 5 5: s = 13, w = 1 + 2 + 3 + 20 + 25 = 51, G = 102 / 65 - 1.2 = 0.369.., Gn = 0.4615.., h = 1.15..: t = 1, (1 + 1 + 5) / 3
    assert _read([5.0, 1.0, 5.0, 1.0, 1.0]) == (float(F32(7.0) / F32(3.0)), 1, 0)
    # K even because n < M: four samples in five buckets (one bucket empty, not dropped): MEDIAN takes t = 1, the mean of the middle two
    b = np.array([4.0, 1.0, 100.0, 2.0, 0.0], F32).reshape(5, 1, 1, 1) * np.ones((1, 1, 1, 3), F32)
    out, t, dropped = ref.robust(b, 0, 4, ref.MEDIAN)
    assert (float(out[0, 0, 0]), int(t[0, 0, 0]), int(dropped[0, 0, 0])) == (3.0, 1, 0)
    out, t, _ = ref.robust(b, 3, 4, ref.MEDIAN)  # first_sample 3: bucket 2 is the empty one, 4 1 2 0 are left: (1 + 2) / 2
    assert (float(out[0, 0, 0]), int(t[0, 0, 0])) == (1.5, 1)
    # MEDIAN and TRIM clamped to (K - 1) / 2
    seven = [7.0, 1.0, 2.0, 3.0, 4.0, 5.0, 600.0]
    assert _read(seven, ref.MEDIAN) == (4.0, 3, 0)
    assert _read(seven, ref.TRIM, 0) == (float(F32(622.0) / F32(7.0)), 0, 0)
    assert _read(seven, ref.TRIM, 1) == (float(F32(21.0) / F32(5.0)), 1, 0)
    assert _read(seven, ref.TRIM, 100) == (4.0, 3, 0)
    assert _read([9.0], ref.TRIM, 100) == (9.0, 0, 0) and _read([9.0]) == (9.0, 0, 0)  # K = 1


def test_designed_states_have_the_properties_they_are_built_for():
    for K in (5, 16):
        for target, (lo_t, hi_t) in ((1.0, (0, 1)), (2.0, (1, 2))):
            below, above = ref.means_at_threshold(K, target)
            hb, ha = ref.gini_h(below), ref.gini_h(above)
            print(f"K {K}, threshold {target}: h {hb!r} below, {ha!r} at or above")
            assert hb < target <= ha and target - hb < 2e-6 and ha - target < 5e-7
            assert ha == target or K == 5  # (robust_ref.means_at_threshold: why K = 5 cannot be exactly on it)
            assert (ref.means_readout(below)[1], ref.means_readout(above)[1]) == (lo_t, hi_t)
        for first in (0, 7):
            buckets, total, _, done, _, _ = ref.designed_state(K, 37, 21, first)
            r = ref.read(buckets, total, first, done)
            assert set(np.unique(r["trim"])) >= {0, 1, 2} and r["info"][4] > 10
            assert np.isnan(r["out"]).any() and np.isnan(r["info"][1])  # the all-non-finite column
            m = ref.read(buckets, total, first, done, ref.MEDIAN)
            assert (m["trim"][np.isfinite(buckets).all(0)] == (K - 1) // 2).all()
        buckets, total, first, done, cnt, conv = ref.designed_state(K, 37, 21, 7, counts=True)
        assert set(np.unique(cnt)) == set(range(K + 2)) | {done} and ((cnt == done) == (conv == 0)).all()
        r = ref.read(buckets, total, first, cnt)
        assert np.isnan(r["out"][cnt == 0]).all() and (r["trim"][cnt <= 2] == 0).all()
    # 257 x 256: more than 256 partial sums, the extremes behind pixel 65 536, and a final sum that needs its tail
    buckets, total, first, done, _, _ = ref.big_state()
    r = ref.read(buckets, total, first, done)
    lp = ref.halves_ref.lum32(ref.plain(total, done)).astype(np.float64).reshape(-1)
    lr = ref.halves_ref.lum32(r["out"]).astype(np.float64).reshape(-1)
    assert -(-lp.size // 256) > 256 and int(np.argmax(lp)) > 65536 and int(np.argmax(lr)) > 65536 and int(np.argmax(lr)) != int(np.argmax(lp))
    assert all(np.isfinite(r["info"][:4])) and r["info"][4] == 0 and r["info"][2] > 0.5
    for lum in (lp, lr):
        assert noise_tree_ref.tree_sum(lum, tail=False) != noise_tree_ref.tree_sum(lum)
    assert r["trim"][255, 3].tolist() == [2, 2, 2] and int((r["trim"] > 0).sum()) == 3 and np.flatnonzero(r["trim"].reshape(-1, 3).any(1))[0] > 65536


def test_what_the_estimator_is_and_is_not():
    """Orderings only; the figures are printed and recorded in DESIGN.md "Sample buckets" and in the header."""
    rows = {}
    for n, M in ((64, 5), (1024, 9)):
        truth, frames = ref.firefly_frames(37, 21, n)
        e = rows[n] = ref.estimator_errors(truth, frames, M)
        print(f"firefly frame, n {n}, M {M}: RMSE mean {e['mean']:.3f}, GINI {e['gini']:.3f}, MEDIAN {e['median']:.3f}; energy removed "
              f"{e['info'][2]:.3f} (GINI) {e['info_median'][2]:.3f} (MEDIAN); frame mean {e['values'][0]:.3f} plain, {e['values'][1]:.3f} GINI, {e['values'][2]:.3f} truth")
        assert e["gini"] < e["mean"] and e["info"][2] > 0 and e["info_median"][2] > 0
    assert rows[64]["median"] < rows[64]["mean"] and rows[1024]["median"] > rows[1024]["mean"]
    # where EVERY pixel is heavy-tailed at a low count the order is the opposite: this is not a denoiser
    truth, frames = ref.synthetic_frames(37, 21, 16)
    import denoise_ref
    import noise_ref
    assert np.array_equal((noise_ref.accumulate(frames)[0] / F32(16)).astype(F32), denoise_ref.synthetic(37, 21)[1])  # the suite's own samples
    e = ref.estimator_errors(truth, frames, 5)
    print(f"heavy-tailed frame, n 16, M 5: RMSE mean {e['mean']:.3f}, GINI {e['gini']:.3f}, MEDIAN {e['median']:.3f}; energy removed {e['info'][2]:.3f}")
    assert e["mean"] < e["gini"] < e["median"] and e["info"][2] > 0
