"""The selected strength without a GPU: the new symbols and struct layouts against the C compiler, rt_select_check through ctypes on every
edge of its ranges, csrc/rt_select_plan.h as a stand-alone program under AddressSanitizer + UBSan, and the designed inputs of
tests/select_ref.py: that each has the property it exists for, on the reference alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import select_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rt_select_check", "rt_accum_denoise_select", "rt_debug_denoise_select", "rt_debug_select_chain"]


def test_symbols_and_struct_layouts_match_the_c_compiler(rt, tmp_path):
    f = rt._ffi
    lib = f.load_gpu_library()
    assert lib.rt_abi_version() == 11 == f.EXPECTED_ABI  # only symbols and two structs were added
    for n in NEW_SYMBOLS:
        assert n in f.GPU_SYMBOLS and hasattr(lib, n), n
    sf, nf = [n for n, _ in f.RtSelect._fields_], [n for n, _ in f.RtSelectInfo._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtow_mi355x_debug.h"\n'
                   'int main(void){int (*a)(const RtSelect*) = rt_select_check;\n'
                   'int (*b)(RtCtx*, const RtSelect*, float*, uint8_t*, uint8_t*, float*, RtSelectInfo*) = rt_accum_denoise_select;\n'
                   'int (*c)(RtCtx*, uint32_t, uint32_t, const float*, const float*, const float*, const float*, const uint32_t*, uint32_t, uint32_t,\n'
                   '         const RtSelect*, float*, uint8_t*, float*, RtSelectInfo*, uint32_t, float*, float*) = rt_debug_denoise_select;\n'
                   'int (*d)(RtCtx*, uint32_t) = rt_debug_select_chain;\n'
                   'printf("%zu' + " %zu" * (len(sf) + 1 + len(nf)) + ' %d %u %u %u\\n", sizeof(RtSelect), ' +
                   ", ".join("offsetof(RtSelect, %s)" % n for n in sf) + ", sizeof(RtSelectInfo), " +
                   ", ".join("offsetof(RtSelectInfo, %s)" % n for n in nf) +
                   ', (a != 0) + (b != 0) + (c != 0) + (d != 0), RT_SELECT_MAX, RT_SELECT_MAX_WINDOW, RT_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", os.path.dirname(f.GPU_LIB_PATH),
                    "-l:librtow_mi355x.so", "-Wl,-rpath," + os.path.dirname(f.GPU_LIB_PATH), "-Wl,--allow-shlib-undefined"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S, I = f.RtSelect, f.RtSelectInfo
    want = [C.sizeof(S)] + [getattr(S, n).offset for n in sf] + [C.sizeof(I)] + [getattr(I, n).offset for n in nf] + [4, f.SELECT_MAX, f.SELECT_MAX_WINDOW, 11]
    assert got == want and (C.sizeof(S), C.sizeof(I)) == (40, 72)
    assert sf == ["n_strengths", "strength", "radius", "patch", "error_radius", "blend_radius", "reserved"]
    assert nf == ["est_mse", "est_mse_selected", "chosen", "usable", "best", "reserved"]


def test_select_check_accepts_and_refuses_exactly_the_edges(rt):
    f = rt._ffi
    ok = lambda **kw: rt.select_check(rt.make_select(**kw))
    assert rt.select_check(None) and ok()  # NULL: the defaults; and the defaults written out
    d = rt.make_select()
    assert (d.n_strengths, [np.float32(x) for x in d.strength][:3], d.radius, d.patch, d.error_radius, d.blend_radius, d.reserved) == \
        (3, [np.float32(x) for x in (0.7, 1.0, 1.4)], 5, 1, 0, 1, 0) and f.SELECT_DEFAULT_STRENGTHS == (0.7, 1.0, 1.4)
    # K = 2 .. 4
    assert not ok(strengths=[0.5]) and ok(strengths=[0.5, 1.0]) and ok(strengths=[0.5, 1.0, 1.5]) and ok(strengths=[0.5, 1.0, 1.5, 2.0])
    for K in (0, 1, 5, 2 ** 32 - 1):
        s = rt.make_select(ref.FOUR_STRENGTHS)
        s.n_strengths = K
        assert not rt.select_check(s), K
    with pytest.raises(ValueError):
        rt.make_select(strengths=[0.1, 0.2, 0.3, 0.4, 0.5])
    # finite, > 0, strictly increasing — over the first K only
    for bad in (0.0, -0.5, float("inf"), float("-inf"), float("nan")):
        for j in range(4):
            s = rt.make_select(ref.FOUR_STRENGTHS)
            s.strength[j] = bad
            assert not rt.select_check(s), (bad, j)
            s.n_strengths = 2
            assert rt.select_check(s) == (j >= 2), (bad, j)
    assert not ok(strengths=[0.7, 0.7]) and not ok(strengths=[0.7, 0.45]) and not ok(strengths=[0.45, 1.0, 0.7])
    assert ok(strengths=[np.nextafter(np.float32(0), np.float32(1)), 3e38])  # the smallest subnormal and a large finite one
    # radius 1 .. 10, patch 0 .. 3, S and T 0 .. 4, reserved 0
    assert [ok(radius=r) for r in (0, 1, f.DENOISE_MAX_RADIUS, f.DENOISE_MAX_RADIUS + 1)] == [False, True, True, False]
    assert [ok(patch=p) for p in (0, f.DENOISE_MAX_PATCH, f.DENOISE_MAX_PATCH + 1)] == [True, True, False]
    assert [ok(error_radius=w) for w in (0, f.SELECT_MAX_WINDOW, f.SELECT_MAX_WINDOW + 1)] == [True, True, False]
    assert [ok(blend_radius=w) for w in (0, f.SELECT_MAX_WINDOW, f.SELECT_MAX_WINDOW + 1)] == [True, True, False]
    s = rt.make_select()
    s.reserved = 1
    assert not rt.select_check(s)


def test_select_plan_header_under_asan_ubsan(tmp_path):
    """csrc/rt_select_plan.h compiled into tests/select_plan_main.cpp with AddressSanitizer + UBSan: every section made its checks, none
    failed and no sanitizer reported."""
    exe = str(tmp_path / "select_plan_san")
    c = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-Wall", "-Wextra",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray_tracing_in_one_weekend_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "select_plan_main.cpp")], capture_output=True, text=True, timeout=600)
    if c.returncode != 0 and "sanitize" in c.stderr + c.stdout and "cannot find" in c.stderr + c.stdout:
        pytest.skip("sanitizer runtime not available")
    assert c.returncode == 0, c.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l[0] for l in lines] == ["check", "windows", "layout", "ok"]
    assert all(int(l[1]) > 0 for l in lines[:-1])


# ---- the designed inputs, on the reference alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [3, 5])
def test_synthetic_halves_use_every_candidate_and_blend(radius):
    halves, first, done, _ = ref.synthetic_halves()
    w = ref.select(halves, first, done, radius=radius)
    npix = w["index"].size
    shares = [n / npix for n in w["info"]["chosen"]]
    mixed = float(((w["W"] != 0).sum(0) >= 2).mean())
    print(f"R {radius}: shares {shares}, pixels with two or more candidates in the blend {mixed:.3f}, info {w['info']}")
    assert sum(w["info"]["chosen"]) == npix == w["info"]["usable"] and min(shares) >= 0.05 and mixed >= 0.10
    assert (w["W"].sum(0) == 9).all() and np.isfinite(w["out"]).all() and np.isfinite(w["est"]).all()


def test_kernel_halves_tie_and_have_unusable_pixels():
    """R 1, F 1, S 1: inside the constant left half of the v = 0 block every weight is 0 or 1 whatever the strength, so the candidates agree
    in every bit over whole windows."""
    halves, first, done, _ = ref.kernel_halves()
    w = ref.select(halves, first, done, radius=1, patch=1, S=1)
    B, U = np.array(w["B"]), w["U"]
    tie = np.all(B == B[-1], axis=0) & (U > 0)
    print(f"exact ties {int(tie.sum())}, unusable {int((~w['usable']).sum())}, windows with 0 < U < 9: {int(((U > 0) & (U < 9)).sum())}, U = 0: {int((U == 0).sum())}")
    assert tie.sum() >= 1 and (w["index"][tie] == 3).all()
    assert (~w["usable"]).sum() >= 1 and ((U > 0) & (U < 9)).sum() >= 1
    assert np.isnan(w["out"]).any() and np.isinf(w["out"]).any()  # the non-finite sample travels, as "Half buffers" says


@pytest.mark.parametrize("first", [4, 7])
def test_adaptive_pixels_without_a_variance_are_unusable(first):
    halves, first, done, cnt, _ = ref.adaptive_state(first)
    w = ref.select(halves, first, cnt)
    low = (w["nh"][0] < 2) | (w["nh"][1] < 2)
    assert low.sum() >= 4 and not w["usable"][low].any() and w["info"]["usable"] == int(w["usable"].sum()) < cnt.size


def test_blind_windows_give_the_last_candidate_and_a_nan():
    halves, first, done, cnt, _ = ref.blind_state()
    w = ref.select(halves, first, cnt)
    blind = w["U"] == 0
    assert blind.sum() >= 1 and np.isnan(w["est"][blind]).all() and not np.isnan(w["est"][~blind]).any() and (w["index"][blind] == 3).all()
    all_blind = ref.select(halves, first, np.ones_like(cnt))  # no pixel has a variance: usable = 0, NaN figures, best = K - 1
    i = all_blind["info"]
    assert i["usable"] == 0 and all(x != x for x in i["est_mse"]) and i["est_mse_selected"] != i["est_mse_selected"] and i["best"] == 3 and i["chosen"] == [0, 0, 0, cnt.size]
