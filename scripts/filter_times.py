"""What a tracked pixel filter costs an add, and what it buys: python scripts/filter_times.py [--size 1920x1080 --spp 64 --reps 5
--kinds none,box,tent,gaussian,mitchell,blackman-harris --lib PATH --quality]
One JSON line.  TIMES: sphere_scene (config 2's scene), one rt_accum_add of --spp samples per variant and repetition, the variants taking
turns inside every repetition after one warm-up turn; the figure is RtStats.seconds_device, the HIP events around the add.  Per variant
"ms" (median), "min" and "spread" (75th minus 25th percentile); per filter "cost ms" = its median minus that of "none", and "share" = cost /
the median of "none".  --lib PATH loads another build of librtow_mi355x.so through ctypes alone — a build without the filter API runs
--kinds none, which is how the untracked add is held against the commit before: it launches nothing new, so the two must agree within the
spread reported here.  QUALITY (--quality): test_sphere's two spheres over a checker ground at 256 x 128, 16 spp under each filter against
a 4096-spp box render of 4x the resolution, box-downsampled: "rmse" of the linear image, and "high band", the share of the error's spectral
energy (luminance, 2-D FFT) beyond half the output's Nyquist frequency on either axis — where what the scene holds above Nyquist folds to
as aliasing rather than as a blur of the picture."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ray_tracing_in_one_weekend_amd as rt  # noqa: E402
from ray_tracing_in_one_weekend_amd import _ffi  # noqa: E402

KINDS = ("box", "tent", "gaussian", "mitchell", "blackman-harris")
ap = argparse.ArgumentParser()
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--kinds", default="none," + ",".join(KINDS))
ap.add_argument("--lib", default=_ffi.GPU_LIB_PATH)
ap.add_argument("--quality", action="store_true")
args = ap.parse_args()
rt.register_default_images()
out = {}


def times():
    lib = C.CDLL(args.lib)  # bound by hand: a build from before the filter API has every symbol used for "none"
    vp = C.c_void_p
    lib.rt_build_id.restype = C.c_char_p
    lib.rt_last_error.restype, lib.rt_last_error.argtypes = C.c_char_p, [vp]
    lib.rt_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.rt_scene_upload.argtypes = [vp, C.POINTER(_ffi.RtFlatScene)]
    lib.rt_accum_begin.argtypes = [vp, C.POINTER(_ffi.RtCamera), C.POINTER(_ffi.RtParams), C.c_uint32]
    lib.rt_accum_add.argtypes = [vp, C.c_uint32, C.POINTER(_ffi.RtStats)]
    lib.rt_accum_end.argtypes = [vp]
    lib.rt_ctx_destroy.argtypes, lib.rt_ctx_destroy.restype = [vp], None

    def check(ctx, rc, what):
        if rc != 0:
            raise SystemExit(f"{what} failed ({rc}): {lib.rt_last_error(ctx).decode()}")
    kinds = args.kinds.split(",")
    if any(k != "none" for k in kinds):
        lib.rt_accum_track_filter.argtypes = [vp, C.POINTER(_ffi.RtPixelFilter)]
    nx, ny = (int(v) for v in args.size.split("x"))
    scene = rt.Scene.build("sphere_scene", nx / ny)
    prm = rt.make_params(nx, ny, args.spp, max_depth=50, seed=95)
    cam = scene.camera
    ctx = vp()
    check(None, lib.rt_ctx_create(0, C.byref(ctx)), "rt_ctx_create")
    check(ctx, lib.rt_scene_upload(ctx, scene.flat_ptr), "rt_scene_upload")
    ms = {k: [] for k in kinds}
    for rep in range(args.reps + 1):
        for k in kinds:
            check(ctx, lib.rt_accum_begin(ctx, C.byref(cam), C.byref(prm), 0), "rt_accum_begin")
            if k != "none":
                flt = rt.make_pixel_filter(k)
                check(ctx, lib.rt_accum_track_filter(ctx, C.byref(flt)), "rt_accum_track_filter")
            st = _ffi.RtStats()
            check(ctx, lib.rt_accum_add(ctx, args.spp, C.byref(st)), "rt_accum_add")
            ms[k].append(st.seconds_device * 1e3)
    lib.rt_accum_end(ctx)
    lib.rt_ctx_destroy(ctx)
    res = {"build": lib.rt_build_id().decode(), "frame": args.size, "spp": args.spp, "reps": args.reps}
    for k, v in ms.items():
        v = sorted(v[1:])
        res[k] = {"ms": round(statistics.median(v), 4), "min": round(v[0], 4), "spread": round(v[(3 * len(v)) // 4] - v[len(v) // 4], 4)}
    if "none" in res:
        for k in kinds:
            if k != "none":
                res[k]["cost ms"] = round(res[k]["ms"] - res["none"]["ms"], 4)
                res[k]["share"] = round(res[k]["cost ms"] / res["none"]["ms"], 4)
    return res


def checker_scene(aspect):
    """test_sphere (demo_scene.rs:229-244) with a checker on the ground: edges finer than a pixel towards the horizon"""
    f = _ffi
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    ground = s.material(f.MAT_LAMBERT, tex0=s.checker_tex((0.1, 0.1, 0.1), (0.9, 0.9, 0.9)))
    grey = s.material(f.MAT_LAMBERT, tex0=s.constant_tex((0.5, 0.5, 0.5)))
    s.sphere((0.0, -100.5, -1.0), 100.0, ground, "Ground")
    s.sphere((0.0, 0.0, -1.0), 0.5, grey, "Test")
    s.set_camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0, 1, 0), 90.0, aspect)
    s.finish()
    return s


def quality():
    nx, ny, up, spp, ref_spp = 256, 128, 4, 16, 4096
    scene = checker_scene(nx / ny)
    r = rt.Renderer(0)
    r.upload(scene)
    r.accum_begin(scene.camera, rt.make_params(nx * up, ny * up, 512, max_depth=50, seed=7))
    for _ in range(ref_spp // 512):
        r.accum_add(512)
    hi = r.accum_read()[0].astype(np.float64)
    ref = hi.reshape(ny, up, nx, up, 3).mean(axis=(1, 3))
    lum = lambda x: 0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]
    fy, fx = np.abs(np.fft.fftfreq(ny))[:, None], np.abs(np.fft.fftfreq(nx))[None, :]
    high = (fy > 0.25) | (fx > 0.25)  # beyond half of Nyquist (0.5 cycles per pixel) on either axis
    res = {"build": rt._ffi.load_gpu_library().rt_build_id().decode(), "frame": f"{nx}x{ny}", "spp": spp, "reference": f"{ref_spp} spp box at {up}x, box-downsampled"}
    for k in KINDS:
        r.accum_begin(scene.camera, rt.make_params(nx, ny, spp, max_depth=50, seed=95))
        r.accum_track_filter(rt.make_pixel_filter(k))
        r.accum_add(spp)
        img = r.accum_filtered()[0].astype(np.float64)
        e = img - ref
        E = np.abs(np.fft.fft2(lum(e))) ** 2
        res[k] = {"rmse": round(float(np.sqrt(np.mean(e * e))), 6), "high band": round(float(E[high].sum() / E.sum()), 4),
                  "high band energy": round(float(E[high].sum() / E.size ** 2), 8)}
    r.accum_end()
    r.close()
    return res


out["times"] = times()
if args.quality:
    out["quality"] = quality()
print(json.dumps(out))
