"""Wall time of rt_accum_denoise_select beside K calls of rt_accum_denoise_halves, the code it is built around:
python scripts/select_times.py [--sizes 1920x1080 --reps 10 --strengths 0.45,0.7,1.0,1.4 --flat]
One JSON line: {"build": .., "<nx>x<ny> select plain" and "select fused": median milliseconds around the C call (which ends in its one
synchronise) under either chain of rt_debug_select_chain, "<nx>x<ny> halves x K": the median of the sum of K calls at the K strengths, each
with "min" and "spread" (the 75th minus the 25th percentile), "<nx>x<ny> fused / plain" and "<nx>x<ny> select plain / halves x K": quotients
of the medians, and "<nx>x<ny> chains agree": whether both chains returned the same image bytes}.  The three take turns inside every
repetition, after one warm-up turn, so that they share whatever else the machine is doing.  sphere_scene, 8 samples per pixel, the defaults of a NULL RtSelect unless --strengths; only the f32
image is asked for, into page-locked memory (rt_host_alloc).  For the kernels' own times run it under a kernel trace in a run of its own
(rocprofv3 --kernel-trace --stats -- python scripts/select_times.py --reps 3 --flat plain): --flat CHAIN runs the selection alone under that
chain, so that every k_denoise dispatch in the trace is the selection's."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ray_tracing_in_one_weekend_amd as rt  # noqa: E402
from ray_tracing_in_one_weekend_amd import _ffi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1920x1080")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--strengths", default=",".join(str(k) for k in _ffi.SELECT_DEFAULT_STRENGTHS))
ap.add_argument("--flat", choices=("plain", "fused"), default=None)
args = ap.parse_args()

rt.register_default_images()
lib = _ffi.load_gpu_library()
strengths = [float(k) for k in args.strengths.split(",")]
sel = rt.make_select(strengths)


def check(ctx, rc, what):
    if rc != 0:
        raise SystemExit(f"{what} failed ({rc}): {lib.rt_last_error(ctx).decode()}")


out = {"build": lib.rt_build_id().decode(), "strengths": strengths}
for size in args.sizes.split(","):
    nx, ny = (int(v) for v in size.split("x"))
    scene = rt.Scene.build("sphere_scene", nx / ny)
    prm = rt.make_params(nx, ny, 8, max_depth=50, seed=95)
    pinned = lib.rt_host_alloc(nx * ny * 3 * 4)
    img = C.cast(pinned, C.POINTER(C.c_float))
    ctx = C.c_void_p()
    check(None, lib.rt_ctx_create(0, C.byref(ctx)), "rt_ctx_create")
    check(ctx, lib.rt_scene_upload(ctx, scene.flat_ptr), "rt_scene_upload")
    cam = scene.camera
    check(ctx, lib.rt_accum_begin(ctx, C.byref(cam), C.byref(prm), 0), "rt_accum_begin")
    check(ctx, lib.rt_accum_track_halves(ctx), "rt_accum_track_halves")
    check(ctx, lib.rt_accum_add(ctx, 8, None), "rt_accum_add")
    CHAINS = {"plain": _ffi.SELECT_CHAIN_PLAIN, "fused": _ffi.SELECT_CHAIN_FUSED}
    hk = f"halves x {len(strengths)}"
    turns = [args.flat] if args.flat else ["plain", "fused"]
    ms = {f"select {c}": [] for c in turns}
    if not args.flat:
        ms[hk] = []
    images = {}
    for rep in range(args.reps + 1):
        for c in turns:
            check(ctx, lib.rt_debug_select_chain(ctx, CHAINS[c]), "rt_debug_select_chain")
            t0 = time.perf_counter()
            rc = lib.rt_accum_denoise_select(ctx, C.byref(sel), img, None, None, None, None)
            ms[f"select {c}"].append((time.perf_counter() - t0) * 1e3)
            check(ctx, rc, "rt_accum_denoise_select")
            if rep == 0:
                images[c] = np.ctypeslib.as_array(img, shape=(nx * ny * 3,)).view(np.uint32).copy()
        if args.flat:
            continue
        t0 = time.perf_counter()
        for k in strengths:
            dn = _ffi.RtDenoise(sel.radius, sel.patch, k, 0)
            rc = rc or lib.rt_accum_denoise_halves(ctx, C.byref(dn), img, None, None, None)
        ms[hk].append((time.perf_counter() - t0) * 1e3)
        check(ctx, rc, "rt_accum_denoise_halves")
    for k, v in ms.items():
        v = sorted(v[1:])
        out[f"{nx}x{ny} {k}"] = round(statistics.median(v), 4)
        out[f"{nx}x{ny} {k} min"] = round(v[0], 4)
        out[f"{nx}x{ny} {k} spread"] = round(v[(3 * len(v)) // 4] - v[len(v) // 4], 4)
    if not args.flat:
        out[f"{nx}x{ny} chains agree"] = bool(np.array_equal(images["plain"], images["fused"]))
        out[f"{nx}x{ny} fused / plain"] = round(out[f"{nx}x{ny} select fused"] / out[f"{nx}x{ny} select plain"], 4)
        out[f"{nx}x{ny} select plain / {hk}"] = round(out[f"{nx}x{ny} select plain"] / out[f"{nx}x{ny} {hk}"], 4)
    lib.rt_accum_end(ctx)
    lib.rt_ctx_destroy(ctx)
    lib.rt_host_free(pinned)
print(json.dumps(out))
