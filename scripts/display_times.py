"""Wall time of rt_accum_read(out_rgb8) without a display and under a manual, a key and a percentile display:
python scripts/display_times.py [--sizes 1920x1080,3840x2160 --reps 20 --parent-lib PATH --flat]
One JSON line: {"build": .., "<nx>x<ny> <configuration>": median milliseconds around the C call (which ends in its one synchronise)}.  The
configurations take turns inside every repetition, after one warm-up turn, so that they share whatever else the machine is doing.
--parent-lib: another build of the library (one from before the display transform will do: only rt_accum_* is called on it) takes its
turn too, as "parent".  out_rgb8 is page-locked (rt_host_alloc); no f32 image is asked for.
--flat: also rt_debug_display of a constant and of a log-uniform plane under the percentile and the key display, three times each — for a
kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/display_times.py --flat --reps 1, in a run of its own): a constant
image puts every pixel of a workgroup into one bin of k_display_stats' histogram."""
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
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--flat", action="store_true")
args = ap.parse_args()

rt.register_default_images()
lib = _ffi.load_gpu_library()
vp = C.c_void_p
libs = {"": lib}
if args.parent_lib:
    parent = C.CDLL(args.parent_lib)
    parent.rt_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    parent.rt_ctx_destroy.argtypes = [vp]
    parent.rt_ctx_destroy.restype = None
    parent.rt_last_error.argtypes, parent.rt_last_error.restype = [vp], C.c_char_p
    parent.rt_scene_upload.argtypes = [vp, C.POINTER(_ffi.RtFlatScene)]
    parent.rt_accum_begin.argtypes = [vp, C.POINTER(_ffi.RtCamera), C.POINTER(_ffi.RtParams), C.c_uint32]
    parent.rt_accum_add.argtypes = [vp, C.c_uint32, C.POINTER(_ffi.RtStats)]
    parent.rt_accum_read.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(_ffi.RtNoise)]
    parent.rt_accum_end.argtypes = [vp]
    libs["parent"] = parent


def check(l, ctx, rc, what):
    if rc != 0:
        raise SystemExit(f"{what} failed ({rc}): {l.rt_last_error(ctx).decode()}")


DISPLAYS = {"none": None, "manual": rt.make_display(1.5, curve="aces", transfer="srgb", dither="bayer8"),
            "key": rt.make_display(0.18, auto="key", curve="aces", transfer="srgb", dither="bayer8"),
            "percentile": rt.make_display(0.8, auto="percentile", percentile=0.99, curve="aces", transfer="srgb", dither="bayer8"),
            "manual gamma2": rt.make_display(1.5, curve="aces", transfer="gamma2", dither="bayer8")}
out = {"build": lib.rt_build_id().decode()}
for size in args.sizes.split(","):
    nx, ny = (int(v) for v in size.split("x"))
    scene = rt.Scene.build("sphere_scene", nx / ny)
    prm = rt.make_params(nx, ny, 2, max_depth=50, seed=95)
    pinned = lib.rt_host_alloc(nx * ny * 3)
    rgb8 = C.cast(pinned, C.POINTER(C.c_uint8))
    ctxs = {}
    for name, l in libs.items():
        ctx = vp()
        check(l, None, l.rt_ctx_create(0, C.byref(ctx)), "rt_ctx_create")
        check(l, ctx, l.rt_scene_upload(ctx, scene.flat_ptr), "rt_scene_upload")
        cam = scene.camera
        check(l, ctx, l.rt_accum_begin(ctx, C.byref(cam), C.byref(prm), 0), "rt_accum_begin")
        check(l, ctx, l.rt_accum_add(ctx, 2, None), "rt_accum_add")
        ctxs[name] = ctx
    turns = [("parent", "parent", None)] if args.parent_lib else []
    turns += [(k, "", d) for k, d in DISPLAYS.items()]
    ms = {k: [] for k, _, _ in turns}
    for rep in range(args.reps + 1):
        for k, which, d in turns:
            l, ctx = libs[which], ctxs[which]
            if which == "":
                check(l, ctx, l.rt_set_display(ctx, C.byref(d) if d is not None else None), "rt_set_display")
            t0 = time.perf_counter()
            rc = l.rt_accum_read(ctx, None, rgb8, None, None)
            ms[k].append((time.perf_counter() - t0) * 1e3)
            check(l, ctx, rc, "rt_accum_read")
    for k in ms:
        out[f"{nx}x{ny} {k}"] = round(statistics.median(ms[k][1:]), 4)
        out[f"{nx}x{ny} {k} min"] = round(min(ms[k][1:]), 4)
    if args.flat:
        rng = np.random.default_rng(1)
        planes = {"flat": np.full((ny, nx, 3), 0.4, np.float32), "random": np.exp2(rng.uniform(-8, 8, (ny, nx, 3))).astype(np.float32)}
        for mode in ("percentile", "key"):
            for pname, plane in planes.items():
                for _ in range(3):
                    info = _ffi.RtDisplayInfo()
                    u8 = np.zeros((ny, nx, 3), np.uint8)
                    t0 = time.perf_counter()
                    rc = lib.rt_debug_display(ctxs[""], nx, ny, plane.ctypes.data_as(C.POINTER(C.c_float)), C.byref(DISPLAYS[mode]),
                                              u8.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info))
                    check(lib, ctxs[""], rc, "rt_debug_display")
                    out[f"{nx}x{ny} debug {mode} {pname}"] = round((time.perf_counter() - t0) * 1e3, 4)
    for name, l in libs.items():
        l.rt_accum_end(ctxs[name])
        l.rt_ctx_destroy(ctxs[name])
    lib.rt_host_free(pinned)
print(json.dumps(out))
