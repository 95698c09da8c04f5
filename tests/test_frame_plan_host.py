"""The host-side frame arithmetic (csrc/rt_frame_plan.h) against brute force, under AddressSanitizer + UBSan: shard rows, the work-buffer
layout, shard capacity, slice sizing, the pixel order and the reciprocals of udiv_inv — what the kernels trust without checking.
tests/frame_plan_main.hip runs it as a stand-alone program: no GPU, no HIP runtime call, not linked against the GPU library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTIONS = ["work_layout", "shard_cap", "slice_fit", "plan_slice_size", "pixel_order_and_shard_rows", "udiv_inv", "frame_gen_params"]


def test_frame_plan_holds_against_brute_force_under_asan_ubsan(tmp_path):
    """Every section of the program made its checks, none failed and no sanitizer reported: status 0."""
    pkg = os.path.join(ROOT, "ray_tracing_in_one_weekend_amd")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    san = "-fsanitize=address,undefined"
    common = ["-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
              "-I", os.path.join(pkg, "csrc")]
    obj, exe = str(tmp_path / "frame_plan_main.o"), str(tmp_path / "frame_plan_san")
    c = subprocess.run([hipcc, "--offload-arch=gfx950", "-Xarch_host", san] + common + ["-c", "-o", obj, os.path.join(ROOT, "tests", "frame_plan_main.hip")],
                       capture_output=True, text=True, timeout=900)
    assert c.returncode == 0, c.stderr[-3000:]
    c = subprocess.run([hipcc, "--offload-arch=gfx950", san, "-o", exe, obj], capture_output=True, text=True, timeout=600)
    if c.returncode != 0 and "sanitize" in c.stderr + c.stdout:
        pytest.skip("sanitizer runtime not available")
    assert c.returncode == 0, c.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l[0] for l in lines] == SECTIONS + ["ok"]
    assert all(int(l[1]) > 0 for l in lines[:-1])
