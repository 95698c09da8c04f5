"""The pixel filters without a GPU: the new symbols and struct layouts against the C compiler, every table entry against an independent f64
evaluation, the reach against a brute-force scan, the check functions on each refusal, csrc/rt_filter_plan.h as a stand-alone program under
AddressSanitizer + UBSan, the .npz round trip of AccumFilter, and two properties of tests/filter_ref.py on the reference alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rt_pixel_filter_check", "rt_pixel_filter_table", "rt_accum_track_filter", "rt_accum_read_filtered", "rt_accum_filter_check",
               "rt_accum_export_filter", "rt_accum_import_filter", "rt_debug_filter_add"]
DEFAULTS = {"box": (0.5, 0.0, 0.0), "tent": (1.0, 0.0, 0.0), "gaussian": (1.5, 0.5, 0.0), "mitchell": (2.0, 1.0 / 3.0, 1.0 / 3.0),
            "blackman-harris": (1.5, 0.0, 0.0)}
f32 = np.float32


def test_symbols_and_struct_layouts_match_the_c_compiler(rt, tmp_path):
    f = rt._ffi
    lib = f.load_gpu_library()
    assert lib.rt_abi_version() == 11 == f.EXPECTED_ABI  # only symbols and two structs were added
    for n in NEW_SYMBOLS:
        assert n in f.GPU_SYMBOLS and hasattr(lib, n), n
    pf = [n for n, _ in f.RtPixelFilter._fields_]
    af = [n for n, _ in f.RtAccumFilter._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x_debug.h"\n'
                   'int main(void){int (*a)(const RtPixelFilter*) = rt_pixel_filter_check;\n'
                   'int (*b)(const RtPixelFilter*, float*, uint32_t*) = rt_pixel_filter_table;\n'
                   'int (*c)(RtCtx*, const RtPixelFilter*) = rt_accum_track_filter;\n'
                   'int (*d)(RtCtx*, float*, uint8_t*, float*) = rt_accum_read_filtered;\n'
                   'int (*e)(const RtAccumFilter*) = rt_accum_filter_check;\n'
                   'int (*g)(RtCtx*, RtAccumFilter*) = rt_accum_export_filter;\n'
                   'int (*h)(RtCtx*, const RtAccumFilter*) = rt_accum_import_filter;\n'
                   'int (*i)(RtCtx*, uint32_t, uint32_t, const float*) = rt_debug_filter_add;\n'
                   'printf("%zu' + " %zu" * (len(pf) + 1 + len(af)) + ' %d %u %u %u %u %u %u %.9g %.9g %u\\n", sizeof(RtPixelFilter), ' +
                   ", ".join("offsetof(RtPixelFilter, %s)" % n for n in pf) + ", sizeof(RtAccumFilter), " +
                   ", ".join("offsetof(RtAccumFilter, %s)" % n for n in af) +
                   ', (a != 0) + (b != 0) + (c != 0) + (d != 0) + (e != 0) + (g != 0) + (h != 0) + (i != 0), RT_FILTER_BOX, RT_FILTER_TENT, RT_FILTER_GAUSSIAN,'
                   ' RT_FILTER_MITCHELL, RT_FILTER_BLACKMAN_HARRIS, RT_FILTER_TABLE, (double)RT_FILTER_MIN_RADIUS, (double)RT_FILTER_MAX_RADIUS, RT_ABI_VERSION);'
                   'return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", os.path.dirname(f.GPU_LIB_PATH),
                    "-l:librtow_mi355x.so", "-Wl,-rpath," + os.path.dirname(f.GPU_LIB_PATH), "-Wl,--allow-shlib-undefined"], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    P, A = f.RtPixelFilter, f.RtAccumFilter
    want = [C.sizeof(P)] + [getattr(P, n).offset for n in pf] + [C.sizeof(A)] + [getattr(A, n).offset for n in af] + [8]
    assert [int(x) for x in got[:len(want)]] == want and (C.sizeof(P), C.sizeof(A)) == (16, 56)
    assert [int(x) for x in got[len(want):len(want) + 6]] == [f.FILTER_BOX, f.FILTER_TENT, f.FILTER_GAUSSIAN, f.FILTER_MITCHELL, f.FILTER_BLACKMAN_HARRIS,
                                                              f.FILTER_TABLE] == [0, 1, 2, 3, 4, 256]
    assert (float(got[-3]), float(got[-2]), int(got[-1])) == (f.FILTER_MIN_RADIUS, f.FILTER_MAX_RADIUS, 11)
    assert pf == ["kind", "radius", "p0", "p1"]
    assert af == ["nx", "rows", "first_sample", "done", "reserved", "frame_id", "filter", "plane"]


def test_make_pixel_filter_defaults(rt):
    for kind, (R, p0, p1) in DEFAULTS.items():
        flt = rt.make_pixel_filter(kind)
        assert (flt.kind, flt.radius, flt.p0, flt.p1) == (ref.KINDS.index(kind), f32(R), f32(p0), f32(p1)) and rt.pixel_filter_check(flt)
    g = rt.make_pixel_filter("gaussian", 2.0, sigma=0.7)
    m = rt.make_pixel_filter("mitchell", 3.0, B=1.0, C=0.0)
    assert (g.radius, g.p0) == (2.0, f32(0.7)) and (m.radius, m.p0, m.p1) == (3.0, 1.0, 0.0)
    with pytest.raises(ValueError):
        rt.make_pixel_filter("lanczos")


FILTERS = [(k, None) for k in ref.KINDS] + [("tent", 0.5), ("tent", 3.0), ("gaussian", 2.75), ("mitchell", 1.5), ("mitchell", 3.0), ("blackman-harris", 0.8),
                                            ("box", 1.5)]


@pytest.mark.parametrize("kind,radius", FILTERS)
def test_every_table_entry_against_an_independent_f64_evaluation(rt, kind, radius):
    """Box, tent and Mitchell are +, -, *, / in a stated order: exact.  The Gaussian and Blackman-Harris go through exp and cos, which two
    libms may round differently in the last bit of the double, so a value close to the middle of two f32 may round either way: 1 ulp."""
    flt = rt.make_pixel_filter(kind, radius)
    table, reach = rt.pixel_filter_table(flt)
    t64, want = ref.table_f64(flt, kind)
    assert table.dtype == f32 and table.shape == (256,) and np.isfinite(table).all()
    ulps = ref.ulp_distance(table, want)
    print(kind, flt.radius, "reach", reach, "largest distance in ulp", int(ulps.max()), "entries off", int((ulps > 0).sum()))
    assert int(ulps.max()) <= (0 if kind in ("box", "tent", "mitchell") else 1)
    if kind not in ("box", "tent", "mitchell"):
        off = ulps > 0  # an entry may differ only where the f64 value lies within a few f64 ulp of the middle between two f32
        lo = np.minimum(table, want).astype(np.float64)
        hi = np.maximum(table, want).astype(np.float64)
        assert (np.abs(t64[off] - 0.5 * (lo[off] + hi[off])) <= 4 * np.spacing(np.abs(t64[off]) + 1.0)).all()
    assert reach == ref.reach_brute(float(flt.radius))


def test_reach_against_a_brute_force_scan(rt):
    for R in (0.5, 0.5000001, 0.75, 1.0, 1.4999999, 1.5, 1.5000001, 2.0, 2.5, 2.5000002, 2.9, 3.0):
        flt = rt.make_pixel_filter("tent", R)
        assert rt.pixel_filter_table(flt)[1] == ref.reach_brute(float(flt.radius)), R
    assert [rt.pixel_filter_table(rt.make_pixel_filter("box", R))[1] for R in (0.5, 1.0, 1.5, 2.0, 2.5, 3.0)] == [0, 1, 1, 2, 2, 3]


def test_check_functions_refuse_each_bad_field(rt):
    lib = rt._ffi.load_gpu_library()
    inv = -rt._ffi.ERR_INVALID
    assert lib.rt_pixel_filter_check(None) == inv and lib.rt_pixel_filter_table(None, None, None) == inv
    good = rt.make_pixel_filter("gaussian")
    assert lib.rt_pixel_filter_check(C.byref(good)) == 0

    def bad(**kw):
        b = rt.RtPixelFilter(good.kind, good.radius, good.p0, good.p1)
        for k, v in kw.items():
            setattr(b, k, v)
        table = np.full(256, 7.0, f32)
        assert lib.rt_pixel_filter_table(C.byref(b), table.ctypes.data_as(C.POINTER(C.c_float)), None) == inv and (table == 7.0).all(), kw
        return lib.rt_pixel_filter_check(C.byref(b)) == inv
    assert bad(kind=5) and bad(kind=2 ** 31)
    for v in (float("nan"), float("inf"), -float("inf")):
        assert bad(radius=v) and bad(p0=v) and bad(p1=v)
    assert bad(radius=0.0) and bad(radius=0.49999997) and bad(radius=3.0000002) and bad(radius=-1.0)
    assert bad(p0=0.0) and bad(p0=-0.5)  # sigma
    assert not rt.pixel_filter_check(None)
    with pytest.raises(rt.RtError):
        rt.pixel_filter_table(rt.make_pixel_filter("tent", 5.0))
    # the snapshot
    assert lib.rt_accum_filter_check(None) == inv
    s = rt.AccumFilter(5, 3, first_sample=3, done=7, frame_id=99, filter=rt.make_pixel_filter("mitchell"))
    assert s.check() and lib.rt_accum_filter_check(C.byref(s.as_struct())) == 0
    for k in range(2):
        fs = s.as_struct()
        fs.reserved[k] = 1
        assert lib.rt_accum_filter_check(C.byref(fs)) == inv
    fs = s.as_struct()
    fs.plane = None
    assert lib.rt_accum_filter_check(C.byref(fs)) == inv
    fs = s.as_struct()
    fs.filter.radius = 0.25
    assert lib.rt_accum_filter_check(C.byref(fs)) == inv
    s.first_sample, s.done = 2 ** 32 - 1 - 7, 7
    assert s.check()
    s.first_sample += 1
    assert not s.check()
    s.first_sample = 3
    s.plane[0, 0] = [np.nan, np.inf, -1.0, 0.0]  # values are not judged
    assert s.check()
    fs = s.as_struct()
    for fn in (lib.rt_accum_export_filter, lib.rt_accum_import_filter):  # the entry points refuse without a context, and need no device to say so
        assert fn(None, C.byref(fs)) == inv
    assert lib.rt_accum_track_filter(None, C.byref(good)) == inv and lib.rt_accum_read_filtered(None, None, None, None) == inv
    assert lib.rt_debug_filter_add(None, 0, 1, None) == inv
    with pytest.raises(ValueError):
        rt.AccumFilter(4, 2, plane=np.zeros((2, 4, 3), f32))


def test_npz_round_trip_is_bit_for_bit(rt, tmp_path):
    rng = np.random.default_rng(5)
    flt = rt.make_pixel_filter("mitchell", 2.5, B=0.1, C=0.7)
    s = rt.AccumFilter(7, 3, first_sample=4, done=2 ** 32 - 5, frame_id=2 ** 64 - 3, plane=rng.random((3, 7, 4), dtype=f32), filter=flt)
    s.plane.view(np.uint32)[1, 0] = [0x7FC01234, 0x80000000, 0xFF800000, 0x00000001]
    path = str(tmp_path / "filter.npz")
    s.save(path)
    assert os.listdir(tmp_path) == ["filter.npz"]
    t = rt.AccumFilter.load(path)
    assert all(getattr(t, k) == getattr(s, k) for k in s._SCALARS)
    assert np.array_equal(t.plane.view(np.uint32), s.plane.view(np.uint32)) and t.check()
    assert bytes(t.filter) == bytes(flt)


def test_filter_plan_header_under_asan_ubsan(tmp_path):
    """csrc/rt_filter_plan.h compiled into tests/filter_plan_main.cpp with AddressSanitizer + UBSan: every section made its checks, none
    failed and no sanitizer reported."""
    exe = str(tmp_path / "filter_plan_san")
    c = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-Wall", "-Wextra",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray_tracing_in_one_weekend_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "filter_plan_main.cpp")], capture_output=True, text=True, timeout=600)
    if c.returncode != 0 and "sanitize" in c.stderr + c.stdout and "cannot find" in c.stderr + c.stdout:
        pytest.skip("sanitizer runtime not available")
    assert c.returncode == 0, c.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l[0] for l in lines] == ["check", "table", "reach", "snapshot", "planes", "ok"]
    assert all(int(l[1]) > 0 for l in lines[:-1])


# ---- the reference alone ------------------------------------------------------------------------------------------------------------------
NX, NY, SEED = 24, 13, 1234


@pytest.mark.parametrize("kind", ref.KINDS)
def test_reference_reconstructs_a_constant_and_its_weight_sum_is_positive(rt, kind):
    """A constant radiance field C, 3 samples: sum.rgb = sum_k fl(w_k C) and sum.w = sum_k w_k, each summed in f32 over the same T terms.
    Every product rounds by at most u |w_k C| and every running sum by at most u times its partial sum's magnitude, u = 2^-24; both sums
    are bounded by A = sum |w_k| (times C), so each carries an error of at most T u A (C) to first order, and the quotient differs from C by
    at most 2 (T + 1) u C A / |W| — derived here from T, A and W of each pixel, nothing measured.  And W > 0 everywhere for the five defaults
    on a full frame of one sample per pixel: the fallback of the read-out is a designed case, not a common one."""
    flt = rt.make_pixel_filter(kind)
    table, D = rt.pixel_filter_table(flt)
    one = ref.add_samples(ref.new_plane(NX, NY), [np.ones((NY, NX, 3), f32)], 0, SEED, table, flt.radius, D)
    print(kind, "1 spp: min W", float(one[..., 3].min()), "max W", float(one[..., 3].max()))
    assert (one[..., 3] > 0).all()
    const = np.array([0.7, 0.25, 3.5], f32)
    frames = [np.broadcast_to(const, (NY, NX, 3)).copy() for _ in range(3)]
    plane = ref.add_samples(ref.new_plane(NX, NY), frames, 5, SEED, table, flt.radius, D)
    c, W = ref.read_out(plane, np.zeros((NY, NX, 3), f32), 3)
    # T and A per pixel: the same walk with |w|, in f64
    T, A = np.zeros((NY, NX)), np.zeros((NY, NX))
    for s in range(3):
        jx, jy = ref.jitter(SEED, NX, NY, 5 + s)
        for dy in range(-D, D + 1):
            for dx in range(-D, D + 1):
                tj0, tj1, ti0, ti1 = max(0, -dy), min(NY, NY - dy), max(0, -dx), min(NX, NX - dx)
                src = (slice(tj0 + dy, tj1 + dy), slice(ti0 + dx, ti1 + dx))
                w, ok = ref.weights(jx[src], jy[src], dx, dy, table, flt.radius)
                T[tj0:tj1, ti0:ti1] += ok
                A[tj0:tj1, ti0:ti1] += np.where(ok, np.abs(w.astype(np.float64)), 0.0)
    assert (W > 0).all() and T.min() >= 3
    bound = 2.0 * (T + 1.0) * 2.0 ** -24 * A / W.astype(np.float64)
    err = np.abs(c.astype(np.float64) - const.astype(np.float64)) / const.astype(np.float64)
    print(kind, "largest relative error", float(err.max()), "smallest bound", float(bound.min()), "terms", int(T.min()), "..", int(T.max()))
    assert (err <= bound[..., None]).all()
    if kind == "box":
        assert np.array_equal(plane[..., 3], np.full((NY, NX), 3, f32)) and (T == 3).all()
