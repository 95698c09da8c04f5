"""AddressSanitizer + UBSan over the host-side scene preparation (csrc/rt_scene_prep.h): the code that makes every index, count, offset
and bound the kernels trust.  tests/scene_prep_main.hip runs it as a stand-alone program: no GPU, no HIP runtime call."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEMO_SCENES = ["sphere_scene", "moving_sphere_scene", "quads_scene", "mesh_scene", "test_sphere", "simple_light_scene", "cornell_box",
               "final_scene", "earth_env_scene", "pbr_sweep_scene"]
INVALID, UNSUPPORTED = -1, -4
REFUSED = {"nan_sphere_centre": INVALID, "xf_parent_not_before_child": INVALID, "sphere_material_out_of_range": INVALID,
           "perlin_permutation_256": INVALID, "image_beyond_texel_pool": INVALID, "medium_without_boundary": INVALID,
           "too_many_media": UNSUPPORTED, "disney_metal_on_rectangle": UNSUPPORTED, "motion_index_out_of_range": INVALID,
           "motion_indices_not_increasing": INVALID, "moving_sphere_below_wrapper": UNSUPPORTED, "quad_u_parallel_to_v": INVALID,
           "planar_kind_2": INVALID, "17_lights": INVALID}


def test_scene_prep_runs_clean_under_asan_ubsan(rt, tmp_path):
    """Every demo scene, an empty scene, an 18-level wrapper chain, 33 media, a wrapped medium, the motion / quad / light sets and the
    sphere grid, then one refused input per rule: the program ends with status 0 (no sanitizer report, no index out of range), the
    refusals carry their codes, and the demo scenes have the world entries rt_debug_world_bounds reports."""
    pkg = os.path.join(ROOT, "ray_tracing_in_one_weekend_amd")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    san = "-fsanitize=address,undefined"
    common = ["-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
              "-I", os.path.join(pkg, "csrc")]
    objs = []
    for src, flags in [(os.path.join(ROOT, "tests", "scene_prep_main.hip"), ["--offload-arch=gfx950", "-Xarch_host", san])] + \
                      [(os.path.join(pkg, "host", f), [san]) for f in ("demo_scene.cpp", "host_capi.cpp", "png_out.cpp")]:
        objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
        c = subprocess.run([hipcc] + flags + common + ["-c", "-o", objs[-1], src], capture_output=True, text=True, timeout=900)
        assert c.returncode == 0, c.stderr[-3000:]
    exe = str(tmp_path / "scene_prep_san")
    c = subprocess.run([hipcc, "--offload-arch=gfx950", san, "-o", exe] + objs + ["-lz"], capture_output=True, text=True, timeout=600)
    if c.returncode != 0 and "sanitize" in c.stderr + c.stdout:
        pytest.skip("sanitizer runtime not available")
    assert c.returncode == 0, c.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    refused = {l[1]: int(l[2]) for l in lines if l[0] == "refuse"}
    assert refused == REFUSED
    valid = {l[0]: [int(x) for x in l[1:]] for l in lines if l[0] != "refuse"}
    for name in ("empty", "chain18", "media33", "rotated_medium", "final_scene/float_texels", "motion", "grid", "grid_motion", "quads",
                 "quads_on_empty", "lights1", "lights16"):
        assert valid[name][0] == 0, name
    for name in DEMO_SCENES:
        rc, n_entries = valid[name][:2]
        assert rc == 0 and n_entries == len(rt.world_bounds(rt.Scene.build(name, 1.5))["entry_id"]), name
