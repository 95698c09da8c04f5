"""The GPU-free side of rt_multi_accum_* (rtow_mi355x.h "progressive accumulation across devices"): the numpy restatement of the row map
(tests/multi_accum_ref.py) against itself, tests/frame_cases.py and tests/accum_state_ref.py; csrc/rt_multi_accum_plan.h as a stand-alone
program under AddressSanitizer + UBSan; and the six functions in the header, the library and _ffi."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import accum_state_ref as ref
import frame_cases
import multi_accum_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1, 1), (7, 3), (16, 11), (24, 27), (40, 75))
BANDS, COUNTS = (1, 4, 8), (1, 2, 3, 8)
CAM12 = [13.0, 2.0, 3.0, 5.3, 0.0, -1.2, 0.1, 3.5, 0.4, -2.0, -1.0, 4.0]
FUNCTIONS = ("rt_multi_accum_begin", "rt_multi_accum_add", "rt_multi_accum_add_adaptive", "rt_multi_accum_join", "rt_multi_accum_import",
             "rt_multi_accum_end")


def _bytes_equal(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def _snapshots_equal(a, b, what):
    for k in ("nx", "rows", "first_sample", "done", "planes", "frame_id"):
        assert a[k] == b[k], (what, k)
    for k in ("sum", "moments", "counts", "converged", "channel_moments", "buckets"):
        _bytes_equal(a.get(k), b.get(k), (what, k))
    for k in ("sum", "moments"):
        _bytes_equal(a["halves"][k], b["halves"][k], (what, "halves", k))


@pytest.mark.parametrize("nx,ny", SIZES)
def test_join_of_split_is_the_frame(nx, ny):
    """join(split(x)) == x as bytes for every band and device count; a shard's rows are frame_cases.shard_rows, in ascending image order,
    and hold exactly the image rows the row formula of the header names."""
    whole = mref.designed(nx, ny, M=16, frame_id=123)
    for band in BANDS + (0,):
        for n in COUNTS:
            shards = mref.split(whole, band, n)
            b = band or 8
            assert [s["rows"] for s in shards] == [frame_cases.shard_rows(ny, b, n, r) for r in range(n)]
            for r, s in enumerate(shards):
                rows = mref.shard_row_map(ny, band, n, r)
                assert list(rows) == [((lj // b) * n + r) * b + lj % b if n > 1 else lj for lj in range(s["rows"])]
                assert ref.state_check(s), (band, n, r)
                _bytes_equal(s["sum"], whole["sum"][rows], (band, n, r))
                _bytes_equal(s["buckets"], whole["buckets"][:, rows], (band, n, r))
                assert s["sum"].shape == (s["rows"], nx, 3) and s["halves"]["moments"].shape == (2, s["rows"], nx, 2)
            owners = np.concatenate([mref.shard_row_map(ny, band, n, r) for r in range(n)])
            assert sorted(owners.tolist()) == list(range(ny))  # every image row in exactly one shard
            _snapshots_equal(mref.join(shards, band, frame_id=123), whole, (band, n))


def test_shard_frame_ids_are_the_shards(rt):
    """split gives every shard accum_state_ref.frame_id of its own (band, n, r) — what rt_accum_frame_id returns for the params device r
    is begun with — and one shard of one is the unsharded frame."""
    whole = mref.designed(16, 11, frame_id=ref.frame_id(CAM12, 16, 11, 50, 1234))
    cam = rt._ffi.RtCamera()
    for k, part in enumerate((cam.origin, cam.horizontal, cam.vertical, cam.lower_left_corner)):
        for c in range(3):
            part[c] = CAM12[3 * k + c]
    for band in (0, 4):
        for n in (1, 2, 3):
            shards = mref.split(whole, band, n, frame=(CAM12, 11, 50, 1234, 0))
            for r, s in enumerate(shards):
                assert s["frame_id"] == ref.frame_id(CAM12, 16, 11, 50, 1234, band or 8, n, r)
                p = rt.make_params(16, 11, 4, max_depth=50, seed=1234, shard_band=band or 8, shard_count=n, shard_id=r)
                assert s["frame_id"] == rt.accum_frame_id(cam, p)
            assert (n > 1) == (shards[0]["frame_id"] != whole["frame_id"])
            assert len({s["frame_id"] for s in shards}) == n


def test_designed_snapshot_is_what_the_gpu_tests_need():
    """The designed frame: accepted by state_check, every finite value distinct within its plane, NaNs with payloads, both infinities and
    -0.0 in the float planes, converged and active pixels, counts below done among the converged."""
    st = mref.designed(24, 27, M=3)
    assert ref.state_check(st) and st["planes"] == ref.COUNTS | ref.CHANNELS
    for a in (st["sum"], st["moments"], st["channel_moments"], st["halves"]["sum"], st["halves"]["moments"], st["buckets"]):
        bits = a.reshape(-1).view(np.uint32 if a.dtype == np.float32 else np.uint64)
        assert len(np.unique(bits)) == bits.size
        assert np.isnan(a).sum() == 3 and np.isposinf(a).sum() == 1 and np.isneginf(a).sum() == 1
        assert ((a == 0) & np.signbit(a)).sum() == 1
    assert 0 < st["converged"].sum() < st["converged"].size and (st["counts"][st["converged"] == 0] == st["done"]).all()
    assert (st["counts"][st["converged"] == 1] < st["done"]).any()


def test_multi_accum_plan_under_asan_ubsan(tmp_path):
    """csrc/rt_multi_accum_plan.h compiled into tests/multi_accum_plan_main.cpp with AddressSanitizer + UBSan and run as a child: every
    section made its checks, none failed and no sanitizer reported."""
    main = os.path.join(ROOT, "tests", "multi_accum_plan_main.cpp")
    exe = str(tmp_path / "multi_accum_plan_san")
    c = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-Wall", "-Wextra",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray_tracing_in_one_weekend_amd", "csrc"), "-o", exe, main],
                       capture_output=True, text=True, timeout=600)
    if c.returncode != 0 and "sanitize" in c.stderr + c.stdout and "cannot find" in c.stderr + c.stdout:
        pytest.skip("sanitizer runtime not available")
    assert c.returncode == 0, c.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l[0] for l in lines] == ["row_map", "placement", "split", "empty_shard", "ok"]
    assert all(int(l[1]) > 0 for l in lines[:-1])


def test_header_library_and_ffi_know_the_six_functions(rt):
    """The header declares the six functions behind rt_multi_render and the three track flags, the library exports them, _ffi binds them
    with the header's argument counts, and the ABI is still 11."""
    f = rt._ffi
    lib = f.load_gpu_library()
    src = open(os.path.join(ROOT, "include", "rtow_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    at = [code.index("int %s(" % name) for name in FUNCTIONS]
    assert at == sorted(at) and at[0] > code.index("int rt_multi_render(")
    for name in FUNCTIONS:
        args = re.search(r"int %s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert name in f.GPU_SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == len(args.split(",")) and getattr(lib, name).restype is C.c_int, name
    flags = {n: int(v) for n, v in re.findall(r"#define RT_MULTI_TRACK_(\w+)\s+(\d+)u", src)}
    assert flags == {"CHANNELS": f.MULTI_TRACK_CHANNELS, "HALVES": f.MULTI_TRACK_HALVES, "BUCKETS": f.MULTI_TRACK_BUCKETS} == {"CHANNELS": 1, "HALVES": 2, "BUCKETS": 4}
    assert lib.rt_abi_version() == 11 == f.EXPECTED_ABI and "#define RT_ABI_VERSION 11u" in src
    for name in ("accum_begin", "accum_add", "accum_add_adaptive", "accum_join", "accum_import", "accum_end"):
        assert callable(getattr(rt.MultiRenderer, name))
