"""The first-hit features without a GPU: the new symbols and struct layouts against the C compiler, the check functions on each refusal,
csrc/rt_features_plan.h as a stand-alone program under AddressSanitizer + UBSan, the .npz round trip of AccumFeatures, and properties of
tests/features_ref.py on the reference alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import features_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rt_features_check", "rt_accum_track_features", "rt_accum_read_features", "rt_accum_features_check", "rt_accum_export_features",
               "rt_accum_import_features", "rt_debug_features_add"]
f32 = np.float32


def test_symbols_and_struct_layouts_match_the_c_compiler(rt, tmp_path):
    f = rt._ffi
    lib = f.load_gpu_library()
    assert lib.rt_abi_version() == 11 == f.EXPECTED_ABI  # only symbols and three structs were added
    for n in NEW_SYMBOLS:
        assert n in f.GPU_SYMBOLS and hasattr(lib, n), n
    structs = [("RtFeatures", f.RtFeatures), ("RtFeaturePixel", f.RtFeaturePixel), ("RtAccumFeatures", f.RtAccumFeatures)]
    src = tmp_path / "probe.c"
    exprs = []
    for name, S in structs:
        exprs += ["sizeof(%s)" % name] + ["offsetof(%s, %s)" % (name, n) for n, _ in S._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x_debug.h"\n'
                   'int main(void){int (*a)(const RtFeatures*) = rt_features_check;\n'
                   'int (*b)(RtCtx*, const RtFeatures*) = rt_accum_track_features;\n'
                   'int (*c)(RtCtx*, float*, float*, float*, float*, float*) = rt_accum_read_features;\n'
                   'int (*d)(const RtAccumFeatures*) = rt_accum_features_check;\n'
                   'int (*e)(RtCtx*, RtAccumFeatures*) = rt_accum_export_features;\n'
                   'int (*g)(RtCtx*, const RtAccumFeatures*) = rt_accum_import_features;\n'
                   'int (*h)(RtCtx*, uint32_t, uint32_t) = rt_debug_features_add;\n'
                   'printf("' + "%zu " * len(exprs) + '%d %u %u %u\\n", ' + ", ".join(exprs) +
                   ', (a != 0) + (b != 0) + (c != 0) + (d != 0) + (e != 0) + (g != 0) + (h != 0), RT_FEATURES_MIN_STRIDE, RT_FEATURES_MAX_STRIDE, RT_ABI_VERSION);'
                   'return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", os.path.dirname(f.GPU_LIB_PATH),
                    "-l:librtow_mi355x.so", "-Wl,-rpath," + os.path.dirname(f.GPU_LIB_PATH), "-Wl,--allow-shlib-undefined"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, S in structs:
        want += [C.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_]
    assert got == want + [7, f.FEATURES_MIN_STRIDE, f.FEATURES_MAX_STRIDE, 11]
    assert (C.sizeof(f.RtFeatures), C.sizeof(f.RtFeaturePixel), C.sizeof(f.RtAccumFeatures)) == (8, 64, 48)
    # the numpy record of a pixel is the C struct, field for field
    assert rt.FEATURE_PIXEL.itemsize == 64 and ref.PIXEL == rt.FEATURE_PIXEL
    assert [(n, rt.FEATURE_PIXEL.fields[n][1]) for n in rt.FEATURE_PIXEL.names] == [(n, getattr(f.RtFeaturePixel, n).offset) for n, _ in f.RtFeaturePixel._fields_]


def test_check_functions_refuse_each_bad_field(rt):
    f = rt._ffi
    lib = f.load_gpu_library()
    inv = -f.ERR_INVALID
    assert lib.rt_features_check(None) == inv and lib.rt_accum_features_check(None) == inv
    for stride in range(0, 70):
        assert rt.features_check(stride) == (1 <= stride <= 64), stride
    assert lib.rt_features_check(C.byref(f.RtFeatures(4, 1))) == inv
    good = rt.AccumFeatures(3, 2, first_sample=5, done=7, frame_id=11, stride=4)
    assert good.check()
    for kw in (dict(stride=0), dict(stride=65), dict(first_sample=2 ** 32 - 1, done=1)):
        assert not rt.AccumFeatures(3, 2, **{**dict(first_sample=5, done=7, frame_id=11, stride=4), **kw}).check(), kw
    assert rt.AccumFeatures(3, 2, first_sample=2 ** 32 - 2, done=1).check()
    st = good.as_struct()
    st.reserved[1] = 1
    assert lib.rt_accum_features_check(C.byref(st)) == inv
    st = good.as_struct()
    st.plane = None
    assert lib.rt_accum_features_check(C.byref(st)) == inv
    st = good.as_struct()
    st.features.reserved = 1
    assert lib.rt_accum_features_check(C.byref(st)) == inv
    with pytest.raises(ValueError):
        rt.AccumFeatures(3, 2, plane=np.zeros((2, 4), rt.FEATURE_PIXEL))


def _random_samples(rng, S, ny, nx):
    hit = rng.random((S, ny, nx)) > 0.3
    n = rng.normal(size=(S, ny, nx, 3)).astype(f32)
    n[~hit] = 0
    return dict(a=rng.random((S, ny, nx, 3), dtype=f32), n=n, hit=hit, z=np.where(hit, rng.uniform(1, 30, (S, ny, nx)), 0).astype(f32))


def test_npz_round_trip_is_bit_for_bit(rt, tmp_path):
    rng = np.random.default_rng(5)
    plane = ref.accumulate(_random_samples(rng, 4, 3, 7))
    plane["albedo"].view(np.uint32)[1, 0] = [0x7FC01234, 0x80000000, 0xFF800000]
    plane["z2"].view(np.uint64)[2, 3] = 0x7FF8000000000123
    s = rt.AccumFeatures(7, 3, first_sample=4, done=2 ** 32 - 5, frame_id=2 ** 64 - 3, stride=64, plane=plane)
    path = str(tmp_path / "features.npz")
    s.save(path)
    assert os.listdir(tmp_path) == ["features.npz"]
    t = rt.AccumFeatures.load(path)
    assert all(getattr(t, k) == getattr(s, k) for k in s._SCALARS)
    assert t.plane.dtype == rt.FEATURE_PIXEL and ref.same_bits(t.plane, s.plane) and t.check()


def test_features_plan_header_under_asan_ubsan(tmp_path):
    """csrc/rt_features_plan.h compiled into tests/features_plan_main.cpp with AddressSanitizer + UBSan: every section made its checks, none
    failed and no sanitizer reported."""
    exe = str(tmp_path / "features_plan_san")
    c = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-Wall", "-Wextra",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray_tracing_in_one_weekend_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "features_plan_main.cpp")], capture_output=True, text=True, timeout=600)
    if c.returncode != 0 and "sanitize" in c.stderr + c.stdout and "cannot find" in c.stderr + c.stdout:
        pytest.skip("sanitizer runtime not available")
    assert c.returncode == 0, c.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.split("\n")
    sections = {ln.split()[0]: int(ln.split()[1]) for ln in lines if len(ln.split()) == 2}
    assert set(sections) == {"features_check", "accum_features_check", "feature_guide_check", "windows", "sizes"} and all(v > 0 for v in sections.values()), sections
    assert "ok" in lines and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- the reference on itself ------------------------------------------------------------------------------------------------------------
def test_contributing_samples_of_a_window():
    for stride in range(1, 65):
        for first in (0, 1, 5, 63, 64, 65):
            whole = ref.contributing(first, 100, stride)
            assert (whole % stride == 0).all() and len(whole) == len([s for s in range(first, first + 100) if s % stride == 0])
            for cut in (0, 1, 37, 100):
                parts = np.concatenate([ref.contributing(first, cut, stride), ref.contributing(first + cut, 100 - cut, stride)])
                assert np.array_equal(parts, whole)
    assert len(ref.contributing(1, 2, 3)) == 0 and len(ref.contributing(4, 2, 3)) == 0


def test_reference_records_do_not_depend_on_how_a_window_is_cut():
    rng = np.random.default_rng(11)
    fh = _random_samples(rng, 6, 4, 5)
    whole = ref.accumulate(fh)
    part = ref.accumulate({k: v[:2] for k, v in fh.items()})
    part = ref.accumulate({k: v[2:] for k, v in fh.items()}, part)
    assert ref.same_bits(whole, part)
    assert (whole["n_f"] == 6).all() and (whole["n_h"] == fh["hit"].sum(axis=0)).all()
    # a pixel that is not active keeps its record
    active = rng.random((4, 5)) > 0.5
    masked = ref.accumulate({k: v[2:] for k, v in fh.items()}, ref.accumulate({k: v[:2] for k, v in fh.items()}), active)
    first_two = ref.accumulate({k: v[:2] for k, v in fh.items()})
    assert ref.same_bits(masked[~active], first_two[~active]) and ref.same_bits(masked[active], whole[active])


def test_reference_read_out():
    rng = np.random.default_rng(3)
    fh = _random_samples(rng, 8, 3, 4)
    fh["hit"][:, 0, 0] = False  # a pixel of sky
    fh["n"][:, 0, 0], fh["z"][:, 0, 0], fh["a"][:, 0, 0] = 0, 0, 1
    fh["hit"][1:, 0, 1] = False  # one hit only: no depth variance
    out = ref.read_out(ref.accumulate(fh))
    a64 = fh["a"].astype(np.float64)
    assert np.allclose(out["albedo"], a64.mean(axis=0), rtol=1e-6) and np.allclose(out["hit"], fh["hit"].mean(axis=0), rtol=1e-6)
    assert np.allclose(out["var"][..., 0], a64.var(axis=0, ddof=1).sum(axis=-1) / 8, rtol=1e-4, atol=1e-9)
    assert (out["albedo"][0, 0] == 1).all() and (out["normal"][0, 0] == 0).all() and out["depth"][0, 0] == 0 and out["hit"][0, 0] == 0
    assert (out["var"][0, 0] == 0).all() and out["var"][0, 1, 2] == 0 and out["depth"][0, 1] == fh["z"][0, 0, 1]
    empty = ref.read_out(np.zeros((2, 2), ref.PIXEL))
    assert all((v == 0).all() for v in empty.values())


# ---- the reference of the feature-guided filter on itself -----------------------------------------------------------------------------
def _random_features(rng, rows, nx):
    return rng.random((rows, nx, 7)).astype(f32), (rng.random((rows, nx, 3)) * 1e-2).astype(f32)


def test_feature_guide_struct_and_defaults(rt):
    f = rt._ffi
    assert C.sizeof(f.RtFeatureGuide) == 40 and [n for n, _ in f.RtFeatureGuide._fields_][6:8] == ["use_mask", "demodulate"]
    g = rt.make_feature_guide()
    assert (g.k_albedo, g.k_normal, g.k_depth) == (f32(0.6),) * 3 and (g.tau_albedo, g.tau_normal, g.tau_depth) == (f32(1e-3),) * 3
    assert g.use_mask == 7 and g.demodulate == 0 and rt.feature_guide_check(g)
    g = rt.make_feature_guide(("normal",), k=(0.1, 0.2, 0.3), tau=0.0, demodulate=True)
    assert (g.use_mask, g.demodulate, g.k_normal, g.tau_depth) == (2, 1, f32(0.2), 0.0) and rt.feature_guide_check(g)
    for bad in (rt.make_feature_guide(k=0.0), rt.make_feature_guide(tau=-1.0), rt.make_feature_guide(use=8), rt.make_feature_guide(k=float("inf"))):
        assert not rt.feature_guide_check(bad)
    bad = rt.make_feature_guide()
    bad.reserved[1] = 1
    assert not rt.feature_guide_check(bad) and not rt.feature_guide_check(None)
    with pytest.raises(ValueError):
        rt.make_feature_guide(("roughness",))


def test_reference_filter_without_features_is_denoise_ref():
    import denoise_ref
    rng = np.random.default_rng(2)
    for nx, rows, R, F in ((15, 17, 5, 1), (9, 5, 2, 0), (20, 7, 3, 3)):
        c, y, v = denoise_ref.kernel_case(nx, rows)
        fm, fv = _random_features(rng, rows, nx)
        a = ref.denoise_features(c, y, v, fm, fv, R, F, 0.7, ref.guide(use=0))
        b = denoise_ref.denoise(c, y, v, R, F, 0.7)[0]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (nx, rows, R, F)


def test_reference_filter_keeps_the_designed_albedo_step():
    """Under colour noise large against the step, denoise_ref.nlm blurs the albedo step (asserted here, on the reference); the feature
    filter's error against the noiseless truth is strictly lower, with and without demodulation."""
    import denoise_ref
    truth, c, y, v, fm, fv = ref.step_plane()
    mid = c.shape[1] // 2
    plain = denoise_ref.denoise(c, y, v, 5, 1, 1.0)[0]
    step_truth = float(truth[0, mid, 0] - truth[0, mid - 1, 0])
    step_plain = float(plain[:, mid, 0].mean() - plain[:, mid - 1, 0].mean())
    assert step_plain < 0.6 * step_truth, (step_plain, step_truth)  # blurred: the columns at the step moved towards each other
    for use, dm in ((1, False), (7, False), (1, True), (7, True)):
        out = ref.denoise_features(c, y, v, fm, fv, 5, 1, 1.0, ref.guide(use, demodulate=dm))
        assert denoise_ref.rmse(out, truth) < denoise_ref.rmse(plain, truth), (use, dm)
    # normal and depth are constant on this plane: they alone change nothing
    out = ref.denoise_features(c, y, v, fm, fv, 5, 1, 1.0, ref.guide(6))
    assert np.array_equal(out.view(np.uint32), plain.view(np.uint32))


def test_reference_filter_sky_pixels_average_and_a_nan_does_not_spread():
    # two sky pixels (albedo 1, normal 0, depth 0, all variances 0) with different colours and a large colour variance
    c = np.array([[[0.2, 0.2, 0.2], [0.8, 0.8, 0.8]]], f32)
    y, v = c[..., 0].copy(), np.full((1, 2), 1.0, f32)
    fm, fv = np.zeros((1, 2, 7), f32), np.zeros((1, 2, 3), f32)
    fm[..., 0:3] = 1
    out = ref.denoise_features(c, y, v, fm, fv, 1, 0, 1.0, ref.guide(7))
    assert np.allclose(out, 0.5, atol=1e-6)
    # a pixel whose features are NaN (n_f < 2) keeps its value and weighs in no other pixel; so does a NaN colour
    rng = np.random.default_rng(4)
    rows, nx = 7, 9
    c = rng.random((rows, nx, 3)).astype(f32)
    y, v = c.mean(axis=-1).astype(f32), np.full((rows, nx), 0.05, f32)
    fm, fv = _random_features(rng, rows, nx)
    base = ref.denoise_features(c, y, v, fm, fv, 2, 1, 1.0, ref.guide(7))
    fm2, fv2 = fm.copy(), fv.copy()
    fm2[3, 4], fv2[3, 4] = np.nan, np.nan
    out = ref.denoise_features(c, y, v, fm2, fv2, 2, 1, 1.0, ref.guide(7))
    assert np.array_equal(out[3, 4], c[3, 4]) and not np.isnan(out).any()
    far = np.ones((rows, nx), bool)
    far[1:6, 2:7] = False  # beyond the window of (3, 4) nothing changed
    assert np.array_equal(out[far], base[far])
    c2, y2 = c.copy(), y.copy()
    c2[3, 4], y2[3, 4] = np.nan, np.nan
    out = ref.denoise_features(c2, y2, v, fm, fv, 2, 1, 1.0, ref.guide(7, demodulate=True))
    assert np.isnan(out[3, 4]).all() and np.isnan(out).sum() == 3
    # filter_inputs: NaN for all ten where n_f < 2
    plane = np.zeros((1, 2), ref.PIXEL)
    plane["n_f"], plane["albedo"] = [[1, 4]], 2.0
    fm3, fv3 = ref.filter_inputs(plane)
    assert np.isnan(fm3[0, 0]).all() and np.isnan(fv3[0, 0]).all() and (fm3[0, 1, 0:3] == 0.5).all() and not np.isnan(fv3[0, 1]).any()


def test_clamp_of_the_albedo():
    x = np.array([np.nan, -1.0, -0.0, 0.25, 1.0, 4.0, np.inf, -np.inf], f32)
    assert np.array_equal(ref.clamp01(x), np.array([0, 0, 0, 0.25, 1, 1, 1, 0], f32))
