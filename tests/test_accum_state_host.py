"""The accumulation state without a GPU: rt_accum_frame_id and rt_accum_state_check through ctypes without a context, against
tests/accum_state_ref.py; the .npz round trip of AccumState, bit for bit with NaN payloads; the layout of RtAccumState against the C
compiler; the merge of the reference on hand-made values; and csrc/rt_accum_state.h as a stand-alone program under AddressSanitizer +
UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import accum_state_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rt_accum_frame_id", "rt_accum_state_check", "rt_accum_export", "rt_accum_import", "rt_accum_merge"]
CAM12 = [13.0, 2.0, 3.0, 4.5, 0.0, -1.25, 0.0, 2.25, 0.0, -2.0, -1.0, 0.5]


def _camera(rt, c12=CAM12):
    cam = rt.RtCamera()
    for k in range(3):
        cam.origin[k], cam.horizontal[k], cam.vertical[k], cam.lower_left_corner[k] = c12[k], c12[3 + k], c12[6 + k], c12[9 + k]
    return cam


def test_symbols_and_struct_layout_match_the_c_compiler(rt, tmp_path):
    f = rt._ffi
    lib = f.load_gpu_library()
    assert lib.rt_abi_version() == 11 == f.EXPECTED_ABI  # only symbols and one struct were added
    for n in NEW_SYMBOLS:
        assert n in f.GPU_SYMBOLS and hasattr(lib, n), n
    fields = [n for n, _ in f.RtAccumState._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x.h"\n'
                   'int main(void){uint64_t (*a)(const RtCamera*, const RtParams*) = rt_accum_frame_id;\n'
                   'int (*b)(const RtAccumState*) = rt_accum_state_check;\n'
                   'int (*c)(RtCtx*, RtAccumState*) = rt_accum_export;\n'
                   'int (*d)(RtCtx*, const RtAccumState*) = rt_accum_import;\n'
                   'int (*e)(RtCtx*, const RtAccumState*) = rt_accum_merge;\n'
                   'printf("%zu' + " %zu" * len(fields) + ' %u %u %d\\n", sizeof(RtAccumState), ' +
                   ", ".join("offsetof(RtAccumState, %s)" % n for n in fields) +
                   ', RT_ACCUM_STATE_COUNTS, RT_ACCUM_STATE_CHANNELS, (a != 0) + (b != 0) + (c != 0) + (d != 0) + (e != 0));return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", os.path.dirname(f.GPU_LIB_PATH),
                    "-l:librtow_mi355x.so", "-Wl,-rpath," + os.path.dirname(f.GPU_LIB_PATH), "-Wl,--allow-shlib-undefined"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = f.RtAccumState
    want = [C.sizeof(S)] + [getattr(S, n).offset for n in fields] + [f.ACCUM_STATE_COUNTS, f.ACCUM_STATE_CHANNELS, 5]
    assert got == want and C.sizeof(S) == 72
    assert fields == ["nx", "rows", "first_sample", "done", "planes", "reserved", "frame_id", "sum", "moments", "counts", "converged", "channel_moments"]
    assert (ref.COUNTS, ref.CHANNELS) == (f.ACCUM_STATE_COUNTS, f.ACCUM_STATE_CHANNELS)


def test_frame_id_of_the_library_is_the_reference(rt):
    lib = rt._ffi.load_gpu_library()
    cam = _camera(rt)
    base = rt.make_params(40, 20, 7, max_depth=50, seed=1234)
    want = ref.frame_id(CAM12, 40, 20, 50, 1234)
    assert rt.accum_frame_id(cam, base) == want == ref.frame_id_of(cam, base)
    assert lib.rt_accum_frame_id(None, C.byref(base)) == 0 and lib.rt_accum_frame_id(C.byref(cam), None) == 0
    # what does not enter: spp, spp_slice, brute force, the diagnostic bits, the shard fields of an unsharded frame
    same = [dict(spp=1000), dict(spp_slice=3), dict(flags=rt._ffi.FLAG_BRUTE_FORCE), dict(flags=rt._ffi.FLAG_TIME_DEPTHS | rt._ffi.FLAG_PRODUCTION_KERNELS),
            dict(shard_count=1, shard_band=9, shard_id=5), dict(shard_count=0, shard_band=2)]
    for kw in same:
        p = rt.make_params(40, 20, kw.pop("spp", 7), max_depth=50, seed=1234, **kw)
        assert rt.accum_frame_id(cam, p) == want, kw
    # what does, each against the reference and different from the base
    other = [dict(flags=rt._ffi.FLAG_RUSSIAN_ROULETTE), dict(shard_count=2, shard_band=4, shard_id=1), dict(shard_count=2, shard_band=4, shard_id=0),
             dict(shard_count=2, shard_band=0, shard_id=1), dict(seed=1235), dict(seed=2 ** 64 - 1), dict(max_depth=8), dict(max_depth=-1),
             dict(nx=20, ny=40), dict(nx=41)]
    seen = {want}
    for kw in other:
        kw = {**dict(nx=40, ny=20, max_depth=50, seed=1234), **kw}
        p = rt.make_params(kw.pop("nx"), kw.pop("ny"), 7, **kw)
        got = rt.accum_frame_id(cam, p)
        assert got == ref.frame_id_of(cam, p) and got not in seen, kw
        seen.add(got)
    # the camera enters by bit pattern: every one of the 12 floats, -0.0 against 0.0, a NaN payload
    for k in range(12):
        c = list(CAM12)
        c[k] = float(np.nextafter(np.float32(c[k]), np.float32(100.0)))
        got = rt.accum_frame_id(_camera(rt, c), base)
        assert got == ref.frame_id(c, 40, 20, 50, 1234) and got not in seen, k
        seen.add(got)
    c = list(CAM12)
    c[4] = -0.0
    assert rt.accum_frame_id(_camera(rt, c), base) == ref.frame_id(c, 40, 20, 50, 1234) != want
    cam = _camera(rt)
    C.cast(C.byref(cam), C.POINTER(C.c_uint32))[7] = 0x7FC01234  # vertical[1]: a quiet NaN with a payload
    bits = np.array(CAM12, np.float32)
    bits.view(np.uint32)[7] = 0x7FC01234
    data = bits.tobytes() + ref.frame_bytes(CAM12, 40, 20, 50, 1234)[48:]
    assert rt.accum_frame_id(cam, base) == ref.fnv1a64(data)
    # a scene camera, as the GPU tests use it
    scene = rt.Scene.build("test_sphere", 2.0)
    assert rt.accum_frame_id(scene.camera, base) == ref.frame_id_of(scene.camera, base)


def _state(rt, nx, rows, planes, done=7, first=3):
    rng = np.random.default_rng(nx * 1000 + rows * 10 + planes)
    counts = converged = chm = None
    if planes & ref.COUNTS:
        converged = (rng.random((rows, nx)) < 0.4).astype(np.uint8)
        counts = np.where(converged == 1, rng.integers(0, done + 1, (rows, nx)), done).astype(np.uint32)
    if planes & ref.CHANNELS:
        chm = rng.random((rows, nx, 6))
    return rt.AccumState(nx, rows, first, done, planes, 0x0123456789ABCDEF, sum=rng.random((rows, nx, 3), dtype=np.float32),
                         moments=rng.random((rows, nx, 2)), counts=counts, converged=converged, channel_moments=chm)


def _as_dict(s):
    d = {k: getattr(s, k) for k in ("nx", "rows", "first_sample", "done", "planes", "frame_id", "sum", "moments", "channel_moments")}
    d["counts"], d["converged"] = (s.counts, s.converged) if s.adaptive else (None, None)
    d["reserved"] = 0
    return d


def test_state_check_of_the_library_is_the_reference(rt):
    lib = rt._ffi.load_gpu_library()
    assert lib.rt_accum_state_check(None) == -rt._ffi.ERR_INVALID
    for nx, rows in ((0, 0), (1, 1), (257, 1), (40, 20)):
        for planes in range(4):
            s = _state(rt, nx, rows, planes)
            if nx == 0:  # (numpy gives an empty array a pointer; the check reads no element)
                assert ref.state_check(_as_dict(s))
            assert s.check() and ref.state_check(_as_dict(s)), (nx, rows, planes)

    def both(s, st=None, d=None):
        """(library, reference) on a struct / dict derived from s"""
        st = st if st is not None else s.as_struct()
        return lib.rt_accum_state_check(C.byref(st)) == 0, ref.state_check(d if d is not None else _as_dict(s))

    for nx in (1, 257):
        s = _state(rt, nx, 1, 3)
        st = s.as_struct()
        st.reserved = 1
        assert both(s, st, dict(_as_dict(s), reserved=1)) == (False, False)
        for bit in (4, 1 << 31):
            st = s.as_struct()
            st.planes |= bit
            assert both(s, st, dict(_as_dict(s), planes=s.planes | bit)) == (False, False)
        for name in ("sum", "moments", "counts", "converged", "channel_moments"):
            st = s.as_struct()
            setattr(st, name, None)
            assert both(s, st, {**_as_dict(s), name: None}) == (False, False), name
        for drop in (ref.COUNTS, ref.CHANNELS):  # the bit goes, the pointers stay
            st = s.as_struct()
            st.planes &= ~drop
            assert both(s, st, dict(_as_dict(s), planes=s.planes & ~drop)) == (False, False)
        s.first_sample, s.done = 2 ** 32 - 1 - 7, 7
        assert both(s) == (True, True)
        s.first_sample += 1
        assert both(s) == (False, False)
        s.first_sample = 3
        # the invariant of the counts
        s.converged[0, nx - 1], s.counts[0, nx - 1] = 0, 7
        assert both(s) == (True, True)
        for conv, cnt, ok in ((2, 7, False), (255, 7, False), (1, 7, True), (1, 0, True), (1, 8, False), (0, 8, False), (0, 6, False), (0, 7, True)):
            s.converged[0, nx - 1], s.counts[0, nx - 1] = conv, cnt
            assert both(s) == (ok, ok), (conv, cnt)
        # values are not judged
        s.sum[0, 0, 0], s.moments[0, 0, 1], s.channel_moments[0, 0, 5] = np.nan, np.inf, -1.0
        assert both(s) == (True, True)
    # a uniform AccumState that carries informative counts hands none to the library
    u = _state(rt, 5, 2, 0)
    u.counts, u.converged = np.full((2, 5), 7, np.uint32), np.zeros((2, 5), np.uint8)
    st = u.as_struct()
    assert not st.counts and not st.converged and u.check()
    # the entry points refuse without a context, and need no device to say so
    for fn in (lib.rt_accum_export, lib.rt_accum_import, lib.rt_accum_merge):
        assert fn(None, C.byref(st)) == -rt._ffi.ERR_INVALID


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def test_npz_round_trip_is_bit_for_bit(rt, tmp_path):
    for planes in range(4):
        s = _state(rt, 7, 3, planes, done=2 ** 32 - 5, first=4)
        s.frame_id = 2 ** 64 - 3
        # NaN payloads, signed zeros, infinities and denormals travel as bits
        s.sum.view(np.uint32)[0, 0] = [0x7FC01234, 0xFFC00001, 0x7F800001]  # quiet NaNs with payloads, a signalling NaN
        s.sum.view(np.uint32)[0, 1] = [0x80000000, 0x00000001, 0xFF800000]
        s.moments.view(np.uint64)[1, 2] = [0x7FF8DEADBEEF0001, 0xFFF0000000000000]
        if s.channels:
            s.channel_moments.view(np.uint64)[2, 6, 5] = 0x7FF0000000000BAD
        path = str(tmp_path / f"state{planes}.npz")
        s.save(path)
        assert sorted(os.listdir(tmp_path)) == sorted(f"state{k}.npz" for k in range(planes + 1))  # exactly the path, no temporary left
        t = rt.AccumState.load(path)
        for k in ("nx", "rows", "first_sample", "done", "planes", "frame_id"):
            assert getattr(t, k) == getattr(s, k) and isinstance(getattr(t, k), int), k
        for name in ("sum", "moments", "counts", "converged", "channel_moments"):
            a, b = getattr(s, name), getattr(t, name)
            assert (a is None) == (b is None), name
            if a is not None:
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), name
        assert t.check()
        s.done = 1
        s.save(path)  # over an existing checkpoint: replaced as a whole
        assert rt.AccumState.load(path).done == 1 and len(os.listdir(tmp_path)) == planes + 1
    with pytest.raises(ValueError):
        rt.AccumState(4, 2, sum=np.zeros((2, 4, 2), np.float32))


def test_a_failed_save_keeps_the_previous_checkpoint(rt, tmp_path, monkeypatch):
    s = _state(rt, 4, 2, 0)
    path = str(tmp_path / "ck.npz")
    s.save(path)
    before = open(path, "rb").read()

    def boom(*a, **kw):
        raise OSError("disk full")
    monkeypatch.setattr(np, "savez", boom)
    s.done = 99
    with pytest.raises(OSError):
        s.save(path)
    assert open(path, "rb").read() == before and os.listdir(tmp_path) == ["ck.npz"]


def test_merge_of_the_reference_on_hand_made_values():
    """One f32 add per channel sum and one f64 add per moment: values chosen so that a double-precision or fused sum would differ."""
    a = ref.make_state(2, 1, 0, 3, 9, [[[1.0, 16777216.0, 0.1], [0.0, np.inf, np.nan]]], [[1.0, 0.1]], [[2.0, 2.0 ** 53]])
    b = ref.make_state(2, 1, 3, 4, 9, [[[2.0 ** -24, 1.0, 0.2], [-0.0, -np.inf, 1.0]]], [[2.0 ** -53, 0.2]], [[3.0, 1.0]])
    m = ref.merge(a, b)
    assert (m["first_sample"], m["done"], m["planes"]) == (0, 7, 0)
    assert m["sum"].dtype == np.float32 and m["moments"].dtype == np.float64
    assert m["sum"][0, 0].tolist() == [1.0, 16777216.0, float(np.float32(0.1) + np.float32(0.2))]  # the small terms round away in f32
    assert m["sum"][0, 1, 0] == 0.0 and np.isnan(m["sum"][0, 1, 1]) and np.isnan(m["sum"][0, 1, 2])
    assert m["moments"][0, 0].tolist() == [1.0, 5.0] and m["moments"][0, 1].tolist() == [0.1 + 0.2, 2.0 ** 53]
    for bad in (dict(first_sample=4), dict(nx=3), dict(rows=2), dict(frame_id=8), dict(planes=ref.CHANNELS), dict(done=2 ** 32 - 3)):
        with pytest.raises(ValueError, match="invalid"):
            ref.merge(a, dict(b, **bad))
    with pytest.raises(ValueError, match="unsupported"):
        ref.merge(a, dict(b, planes=ref.COUNTS))
    z = ref.make_state(2, 1, 3, 0, 9, np.zeros((1, 2, 3)), np.zeros((1, 2)), np.zeros((1, 2)))
    assert np.array_equal(ref.merge(z, b)["sum"][0, 0], b["sum"][0, 0]) and ref.merge(z, b)["done"] == 4  # 0 + x


def test_accum_state_header_under_asan_ubsan(tmp_path):
    """csrc/rt_accum_state.h compiled into tests/accum_state_main.cpp with AddressSanitizer + UBSan: every section made its checks, none
    failed and no sanitizer reported.  The hash constants in the program are what the Python restatement produces."""
    main = os.path.join(ROOT, "tests", "accum_state_main.cpp")
    consts = dict(re.findall(r"#define RT_TEST_ID_(\w+) (0x[0-9a-f]+)ull", open(main).read()))
    neg = list(CAM12)
    neg[4] = -0.0
    want = {"BASE": ref.frame_id(CAM12, 40, 20, 50, 1234), "RR": ref.frame_id(CAM12, 40, 20, 50, 1234, flags=3),
            "SHARD": ref.frame_id(CAM12, 40, 20, 50, 1234, 4, 2, 1), "SEED": ref.frame_id(CAM12, 40, 20, -1, 0xFEDCBA9876543210),
            "NEGZERO": ref.frame_id(neg, 40, 20, 50, 1234)}
    assert {k: int(v, 16) for k, v in consts.items()} == want
    exe = str(tmp_path / "accum_state_san")
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
    assert [l[0] for l in lines] == ["sizes", "check", "identity", "ok"]
    assert all(int(l[1]) > 0 for l in lines[:-1])


# What each class's file holds, key by key, as the first version of each class wrote it: the scalars as 0-d uint64 in this order, then the
# arrays; an AccumState leaves out the planes it does not hold.
NPZ_SCALARS = {"AccumState": ["nx", "rows", "first_sample", "done", "planes", "frame_id"],
               "AccumHalves": ["nx", "rows", "first_sample", "done", "frame_id"],
               "AccumBuckets": ["nx", "rows", "first_sample", "done", "M", "frame_id"]}
NPZ_ARRAYS = {"AccumState": [("sum", "<f4", (2, 3, 3)), ("moments", "<f8", (2, 3, 2)), ("counts", "<u4", (2, 3)), ("converged", "|u1", (2, 3)),
                             ("channel_moments", "<f8", (2, 3, 6))],
              "AccumHalves": [("sum", "<f4", (2, 2, 3, 3)), ("moments", "<f8", (2, 2, 3, 2))],
              "AccumBuckets": [("sum", "<f4", (5, 2, 3, 3))]}


@pytest.mark.parametrize("cls,absent", [("AccumState", ()), ("AccumState", ("counts", "converged", "channel_moments")), ("AccumState", ("channel_moments",)),
                                        ("AccumHalves", ()), ("AccumBuckets", ())])
def test_npz_keys_and_dtypes_are_the_first_version_s(rt, tmp_path, cls, absent):
    """save writes exactly the listed keys with the listed dtypes, and a file written with plain np.savez from that list loads back."""
    rng = np.random.default_rng(5)
    scalars = dict(nx=3, rows=2, first_sample=2 ** 32 - 9, done=8, frame_id=2 ** 64 - 3)
    planes = (0 if "counts" in absent else ref.COUNTS) | (0 if "channel_moments" in absent else ref.CHANNELS)
    scalars.update({"AccumState": dict(planes=planes), "AccumBuckets": dict(M=5)}.get(cls, {}))
    assert sorted(scalars) == sorted(NPZ_SCALARS[cls])
    arrays = {}
    for name, dt, shape in NPZ_ARRAYS[cls]:
        if name not in absent:
            bits = rng.integers(0, 256, size=int(np.prod(shape)) * np.dtype(dt).itemsize, dtype=np.uint8)
            arrays[name] = bits.view(dt).reshape(shape) if name not in ("counts", "converged") else np.full(shape, 8 * (name == "counts"), dt)
    Class = getattr(rt, cls)
    # 1. what save writes
    path = tmp_path / "saved.npz"
    Class(**scalars, **arrays).save(str(path))
    assert sorted(os.listdir(tmp_path)) == ["saved.npz"]  # (the temporary file is gone)
    with np.load(path) as z:
        assert z.files == NPZ_SCALARS[cls] + [n for n, _, _ in NPZ_ARRAYS[cls] if n not in absent]
        for k in NPZ_SCALARS[cls]:
            assert z[k].dtype == np.uint64 and z[k].shape == () and int(z[k]) == scalars[k], k
        for name, dt, shape in NPZ_ARRAYS[cls]:
            if name not in absent:
                assert z[name].dtype.str == dt and z[name].shape == shape and z[name].tobytes() == arrays[name].tobytes(), name
    # 2. a file made without the class
    plain = tmp_path / "plain.npz"
    np.savez(plain, **{k: np.asarray(scalars[k], dtype=np.uint64) for k in NPZ_SCALARS[cls]}, **arrays)
    for back in (Class.load(str(plain)), Class.load(str(path))):
        for k in NPZ_SCALARS[cls]:
            assert getattr(back, k) == scalars[k], k
        for name, dt, shape in NPZ_ARRAYS[cls]:
            got = getattr(back, name)
            if name in absent:
                assert got is None, name
            else:
                assert got.dtype.str == dt and got.tobytes() == arrays[name].tobytes(), name
        assert back.check()
