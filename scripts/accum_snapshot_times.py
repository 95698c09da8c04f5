"""Wall time of the seven snapshot calls of an accumulation (rt_accum_export / _import / _merge and their _halves and _buckets twins) on one
frame: python scripts/accum_snapshot_times.py [--nx 1920 --ny 1080 --reps 5]
One JSON line: {"build": .., "<call> <what>": median milliseconds around the C call (which ends in its one synchronise), after one warm-up}.
The arrays are pageable numpy arrays that the process has touched.  RTOW_GPU_LIB=<path> measures another build of the library; for the
kernels' own times run it under a kernel trace in a run of its own (rocprofv3 --kernel-trace --stats -- python scripts/accum_snapshot_times.py)."""
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
ap.add_argument("--nx", type=int, default=1920)
ap.add_argument("--ny", type=int, default=1080)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
nx, ny, DONE = args.nx, args.ny, 16

rt.register_default_images()
scene = rt.Scene.build("sphere_scene", nx / ny)
r = rt.Renderer(0)
r.upload(scene)
prm = rt.make_params(nx, ny, DONE, max_depth=50, seed=95)
fid = rt.accum_frame_id(scene.camera, prm)
lib, ctx = r._lib, r._ctx
out = {"build": r.build_id, "nx": nx, "ny": ny}


def timed(name, what, struct, before=None):
    """`name`(ctx, struct) reps + 1 times, `before(k)` in front of each (not timed); the median of all but the first."""
    ms = []
    for k in range(args.reps + 1):
        if before:
            before(k)
        t0 = time.perf_counter()
        rc = getattr(lib, name)(ctx, C.byref(struct))
        ms.append((time.perf_counter() - t0) * 1e3)
        if rc != 0:
            raise SystemExit(f"{name} ({what}) failed ({rc}): {lib.rt_last_error(ctx).decode()}")
    out[f"{name} {what}"] = round(statistics.median(ms[1:]), 4)


def begin(*snapshots):
    r.accum_begin(scene.camera, prm)
    for call, s in snapshots:
        getattr(r, call)(s)


def ones(shape, dt):
    return np.ones(shape, dt)  # (touched pages)


for what, planes in (("plain", 0), ("counts+channels", _ffi.ACCUM_STATE_COUNTS | _ffi.ACCUM_STATE_CHANNELS)):
    full = planes != 0
    state = rt.AccumState(nx, ny, 0, DONE, planes, fid, sum=ones((ny, nx, 3), np.float32), moments=ones((ny, nx, 2), np.float64),
                          counts=np.full((ny, nx), DONE, np.uint32) if full else None, converged=np.zeros((ny, nx), np.uint8) if full else None,
                          channel_moments=ones((ny, nx, 6), np.float64) if full else None)
    st = state.as_struct()
    timed("rt_accum_import", what, st, before=lambda k: begin())
    timed("rt_accum_export", what, st)
    if not full:
        def next_window(k):
            st.first_sample = DONE * (k + 1)
        timed("rt_accum_merge", what, st, before=next_window)
        st.first_sample = 0
plain = rt.AccumState(nx, ny, 0, DONE, 0, fid, sum=ones((ny, nx, 3), np.float32), moments=ones((ny, nx, 2), np.float64))
halves = rt.AccumHalves(nx, ny, 0, DONE, fid, sum=ones((2, ny, nx, 3), np.float32), moments=ones((2, ny, nx, 2), np.float64))
hs = halves.as_struct()
timed("rt_accum_import_halves", "", hs, before=lambda k: begin(("accum_import", plain)))
timed("rt_accum_export_halves", "", hs)
for M in (5, 16):
    buckets = rt.AccumBuckets(nx, ny, M, 0, DONE, fid, sum=ones((M, ny, nx, 3), np.float32))
    bs = buckets.as_struct()
    timed("rt_accum_import_buckets", f"M={M}", bs, before=lambda k: begin(("accum_import", plain)))
    timed("rt_accum_export_buckets", f"M={M}", bs)
r.accum_end()
r.close()
print(json.dumps(out))
