"""Motion blur (rt_set_motion, DESIGN.md "Moving spheres") in numpy float32, every operation rounded once in the kernels' order:
the time of a path from its key, the centre of a moving sphere at that time.  The oracle knows no motion, so this restatement is the
reference of tests/test_motion.py; primary rays and Sphere::hit come from tests/lens_ref.py and tests/golden/np_ref.py."""
import numpy as np

from helpers import ctr_draw

f32 = np.float32
TIME_COUNTER = 254  # counters 0, 1: pixel jitter; 2..253: lens; 254: time; 255: free (DESIGN.md "RNG")


def path_time(keys, shutter_open, shutter_close):
    """tm = fl(open + fl(u * fl(close - open))), u = the f32 draw of counter 254 of the path's key; keys: uint32 [n, 2]"""
    keys = np.asarray(keys, dtype=np.uint32).reshape(-1, 2)
    u = ((ctr_draw(keys[:, 0].astype(np.uint64), keys[:, 1].astype(np.uint64), TIME_COUNTER) >> 8).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)
    span = f32(f32(shutter_close) - f32(shutter_open))
    return (f32(shutter_open) + (u * span).astype(f32)).astype(f32)


def center_at(c0, c1, tm):
    """c(tm) = fl(c0 + fl(tm * dc)) per component, dc = fl(c1 - c0); c0, c1: [3] or [n, 3], tm: scalar or [n] -> float32 [n, 3]"""
    c0, c1 = np.asarray(c0, dtype=f32), np.asarray(c1, dtype=f32)
    dc = (c1 - c0).astype(f32)
    tm = np.atleast_1d(np.asarray(tm, dtype=f32))
    return (c0 + (tm[:, None] * dc).astype(f32)).astype(f32)
