"""What tracked first-hit features cost an add: python scripts/features_times.py [--size 1920x1080 --spp 64 --reps 5
--strides none,1,4,16 --scenes sphere_scene,cornell_box --lib PATH]
One JSON line.  Per scene, one rt_accum_add of --spp samples per variant and repetition, the variants taking turns inside every repetition
after one warm-up turn; the figure is RtStats.seconds_device, the HIP events around the add (k_features runs between them, on the frame's
stream).  Per variant "ms" (median), "min" and "spread" (75th minus 25th percentile); per stride "cost ms" = its median minus that of
"none", "share" = cost / the median of "none", and "us per feature sample and Mpixel".  --lib PATH loads another build of
librtow_mi355x.so through ctypes alone — a build from before the feature API runs --strides none, which is how the untracked add is held
against the commit before: it launches nothing new, so the two must agree within the spread reported here and the box-to-box band the
README quotes.  With the feature API in the library, also "denoise": rt_accum_denoise against rt_accum_denoise_features (R 5, F 1, every
feature, without and with demodulation) on sphere_scene's frame, wall time of the call with no output asked for (its input kernels, the filter
and one synchronisation), taking turns, medians."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ray_tracing_in_one_weekend_amd as rt  # noqa: E402
from ray_tracing_in_one_weekend_amd import _ffi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--strides", default="none,1,4,16")
ap.add_argument("--scenes", default="sphere_scene,cornell_box")
ap.add_argument("--lib", default=_ffi.GPU_LIB_PATH)
args = ap.parse_args()
rt.register_default_images()

lib = C.CDLL(args.lib)  # bound by hand: a build from before the feature API has every symbol used for "none"
vp = C.c_void_p
lib.rt_build_id.restype = C.c_char_p
lib.rt_last_error.restype, lib.rt_last_error.argtypes = C.c_char_p, [vp]
lib.rt_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
lib.rt_scene_upload.argtypes = [vp, C.POINTER(_ffi.RtFlatScene)]
lib.rt_accum_begin.argtypes = [vp, C.POINTER(_ffi.RtCamera), C.POINTER(_ffi.RtParams), C.c_uint32]
lib.rt_accum_add.argtypes = [vp, C.c_uint32, C.POINTER(_ffi.RtStats)]
lib.rt_accum_end.argtypes = [vp]
lib.rt_ctx_destroy.argtypes, lib.rt_ctx_destroy.restype = [vp], None
variants = args.strides.split(",")
if any(v != "none" for v in variants):
    lib.rt_accum_track_features.argtypes = [vp, C.POINTER(_ffi.RtFeatures)]


def check(ctx, rc, what):
    if rc != 0:
        raise SystemExit(f"{what} failed ({rc}): {lib.rt_last_error(ctx).decode()}")


nx, ny = (int(v) for v in args.size.split("x"))
out = {"build": lib.rt_build_id().decode(), "frame": args.size, "spp": args.spp, "reps": args.reps}
ctx = vp()
check(None, lib.rt_ctx_create(0, C.byref(ctx)), "rt_ctx_create")
for name in args.scenes.split(","):
    scene = rt.Scene.build(name, nx / ny)
    prm = rt.make_params(nx, ny, args.spp, max_depth=50, seed=95)
    cam = scene.camera
    check(ctx, lib.rt_scene_upload(ctx, scene.flat_ptr), "rt_scene_upload")
    ms = {v: [] for v in variants}
    for rep in range(args.reps + 1):
        for v in variants:
            check(ctx, lib.rt_accum_begin(ctx, C.byref(cam), C.byref(prm), 0), "rt_accum_begin")
            if v != "none":
                check(ctx, lib.rt_accum_track_features(ctx, C.byref(_ffi.RtFeatures(int(v), 0))), "rt_accum_track_features")
            st = _ffi.RtStats()
            check(ctx, lib.rt_accum_add(ctx, args.spp, C.byref(st)), "rt_accum_add")
            ms[v].append(st.seconds_device * 1e3)
    lib.rt_accum_end(ctx)
    res = {}
    for v, t in ms.items():
        t = sorted(t[1:])
        res[v] = {"ms": round(statistics.median(t), 4), "min": round(t[0], 4), "spread": round(t[(3 * len(t)) // 4] - t[len(t) // 4], 4)}
    if "none" in res:
        for v in variants:
            if v != "none":
                n_feat = len([s for s in range(args.spp) if s % int(v) == 0])
                res[v]["cost ms"] = round(res[v]["ms"] - res["none"]["ms"], 4)
                res[v]["share"] = round(res[v]["cost ms"] / res["none"]["ms"], 4)
                res[v]["us per feature sample and Mpixel"] = round(res[v]["cost ms"] * 1e3 / n_feat / (nx * ny / 1e6), 3)
    out[name] = res
if any(v != "none" for v in variants):
    import time
    lib.rt_accum_denoise.argtypes = [vp, C.POINTER(_ffi.RtDenoise), C.POINTER(C.c_float), C.POINTER(C.c_uint8)]
    lib.rt_accum_denoise_features.argtypes = [vp, C.POINTER(_ffi.RtDenoise), C.POINTER(_ffi.RtFeatureGuide), C.POINTER(C.c_float), C.POINTER(C.c_uint8)]
    scene = rt.Scene.build("sphere_scene", nx / ny)
    prm = rt.make_params(nx, ny, args.spp, max_depth=50, seed=95)
    cam = scene.camera
    check(ctx, lib.rt_scene_upload(ctx, scene.flat_ptr), "rt_scene_upload")
    check(ctx, lib.rt_accum_begin(ctx, C.byref(cam), C.byref(prm), 0), "rt_accum_begin")
    check(ctx, lib.rt_accum_track_features(ctx, C.byref(_ffi.RtFeatures(4, 0))), "rt_accum_track_features")
    check(ctx, lib.rt_accum_add(ctx, args.spp, None), "rt_accum_add")
    ip = None  # no output: the kernels and the one synchronisation
    dn = _ffi.RtDenoise(5, 1, 1.0, 0)
    guides = {"features": rt.make_feature_guide(), "features, demodulated": rt.make_feature_guide(demodulate=True)}
    ms = {"plain": [], **{k: [] for k in guides}}
    for rep in range(args.reps + 1):
        for k in ms:
            t0 = time.perf_counter()
            rc = lib.rt_accum_denoise(ctx, C.byref(dn), ip, None) if k == "plain" else lib.rt_accum_denoise_features(ctx, C.byref(dn), C.byref(guides[k]), ip, None)
            ms[k].append((time.perf_counter() - t0) * 1e3)
            check(ctx, rc, k)
    lib.rt_accum_end(ctx)
    out["denoise"] = {}
    for k, t in ms.items():
        t = sorted(t[1:])
        out["denoise"][k] = {"ms": round(statistics.median(t), 4), "min": round(t[0], 4), "spread": round(t[(3 * len(t)) // 4] - t[len(t) // 4], 4)}
lib.rt_ctx_destroy(ctx)
print(json.dumps(out))
