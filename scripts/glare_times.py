"""Wall time of rt_accum_read(out_rgb8) under a display alone, under a display and a glare with the plain down chain, and with the fused one:
python scripts/glare_times.py [--sizes 1920x1080,3840x2160 --reps 20 --levels 6]
One JSON line: {"build": .., "<nx>x<ny> <configuration>": median milliseconds around the C call (which ends in its one synchronise),
"<nx>x<ny> <configuration> min": the fastest, "<nx>x<ny> <configuration> spread": the 75th minus the 25th percentile of the repetitions,
"<nx>x<ny> glare bytes": the algorithmic traffic of the glare stage, "<nx>x<ny> glare <chain> GB/s": those bytes over the median the
glare adds to the display}.  The configurations take turns inside every repetition, after one warm-up turn, so that they share whatever
else the machine is doing.  The chain is chosen by rt_debug_glare_chain, the glare is the default one with --levels levels.  out_rgb8 is
page-locked (rt_host_alloc); no f32 image is asked for."""
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
ap.add_argument("--sizes", default="1920x1080,3840x2160")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--levels", type=int, default=_ffi.GLARE_DEFAULT_LEVELS)
args = ap.parse_args()

rt.register_default_images()
lib = _ffi.load_gpu_library()
vp = C.c_void_p


def check(ctx, rc, what):
    if rc != 0:
        raise SystemExit(f"{what} failed ({rc}): {lib.rt_last_error(ctx).decode()}")


def glare_bytes(nx, ny, levels):
    """The bytes the definition makes the stage move, 12 per pixel of a level: c read by the bright pass and again by the combine, every
    d_l written once and read by the next level and by its u_l, every u_l written once and read by the level below, `out` written."""
    sizes = [(nx, ny)]
    for _ in range(levels):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    px = [a * b for a, b in sizes]
    total = 2 * px[0] + px[0]                 # c twice, out
    total += sum(3 * p for p in px[1:-1])     # d_l: written, read by D and by u_l
    total += 2 * px[-1]                       # the coarsest d: written, read by its u
    total += sum(2 * p for p in px[1:])       # u_l: written, read once (four taps of it per fine pixel hit the cache)
    return 12 * total


DISPLAY = rt.make_display(1.5, curve="aces", transfer="srgb", dither="bayer8")
GLARE = rt.make_glare(levels=args.levels)
TURNS = (("display", None, _ffi.GLARE_CHAIN_AUTO), ("display + glare plain", GLARE, _ffi.GLARE_CHAIN_PLAIN), ("display + glare fused", GLARE, _ffi.GLARE_CHAIN_FUSED))
out = {"build": lib.rt_build_id().decode(), "levels": args.levels}
for size in args.sizes.split(","):
    nx, ny = (int(v) for v in size.split("x"))
    scene = rt.Scene.build("sphere_scene", nx / ny)
    prm = rt.make_params(nx, ny, 2, max_depth=50, seed=95)
    pinned = lib.rt_host_alloc(nx * ny * 3)
    rgb8 = C.cast(pinned, C.POINTER(C.c_uint8))
    ctx = vp()
    check(None, lib.rt_ctx_create(0, C.byref(ctx)), "rt_ctx_create")
    check(ctx, lib.rt_scene_upload(ctx, scene.flat_ptr), "rt_scene_upload")
    cam = scene.camera
    check(ctx, lib.rt_accum_begin(ctx, C.byref(cam), C.byref(prm), 0), "rt_accum_begin")
    check(ctx, lib.rt_accum_add(ctx, 2, None), "rt_accum_add")
    check(ctx, lib.rt_set_display(ctx, C.byref(DISPLAY)), "rt_set_display")
    ms = {k: [] for k, _, _ in TURNS}
    images = {}
    for rep in range(args.reps + 1):
        for k, g, chain in TURNS:
            check(ctx, lib.rt_set_glare(ctx, C.byref(g) if g is not None else None), "rt_set_glare")
            check(ctx, lib.rt_debug_glare_chain(ctx, chain), "rt_debug_glare_chain")
            t0 = time.perf_counter()
            rc = lib.rt_accum_read(ctx, None, rgb8, None, None)
            ms[k].append((time.perf_counter() - t0) * 1e3)
            check(ctx, rc, "rt_accum_read")
            if rep == 0:
                images[k] = np.ctypeslib.as_array(rgb8, shape=(nx * ny * 3,)).copy()
    out[f"{nx}x{ny} chains agree"] = bool(np.array_equal(images["display + glare plain"], images["display + glare fused"]))
    for k in ms:
        v = sorted(ms[k][1:])
        out[f"{nx}x{ny} {k}"] = round(statistics.median(v), 4)
        out[f"{nx}x{ny} {k} min"] = round(v[0], 4)
        out[f"{nx}x{ny} {k} spread"] = round(v[(3 * len(v)) // 4] - v[len(v) // 4], 4)
    nbytes = glare_bytes(nx, ny, args.levels)
    out[f"{nx}x{ny} glare bytes"] = nbytes
    for chain in ("plain", "fused"):
        added = out[f"{nx}x{ny} display + glare {chain}"] - out[f"{nx}x{ny} display"]
        out[f"{nx}x{ny} glare {chain} ms"] = round(added, 4)
        out[f"{nx}x{ny} glare {chain} GB/s"] = round(nbytes / (added * 1e-3) / 1e9, 1) if added > 0 else None
    lib.rt_accum_end(ctx)
    lib.rt_ctx_destroy(ctx)
    lib.rt_host_free(pinned)
print(json.dumps(out))
