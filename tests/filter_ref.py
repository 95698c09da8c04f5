"""Numpy restatement of "Pixel reconstruction filters" (rtow_mi355x.h): the plane (sum w rgb, sum w) of an accumulation from its per-sample
frames, every operation one f32 operation in the order of the header — samples ascending, dy ascending, dx ascending — and the read-out.
The jitter of a sample is the draws 0 and 1 of its path key (helpers.path_keys, helpers.ctr_draw), as helpers.primary_rays takes them; the
table is the one the library returns (its entries are checked against an f64 evaluation of their own in tests/test_filter_host.py).  Also
the independent f64 profiles and the brute-force reach that test uses."""
import math

import numpy as np

from helpers import ctr_draw, path_keys

f32 = np.float32
KINDS = ("box", "tent", "gaussian", "mitchell", "blackman-harris")
TABLE = 256


def jitter(seed, nx, rows, samp):
    """(jx, jy) [rows, nx] f32 of sample `samp` of every pixel: (u32 >> 8) * 2^-24 of the draws 0 and 1 of path_key(seed, j * nx + i, samp)"""
    pix = np.arange(nx * rows, dtype=np.uint64)
    keys = path_keys(int(seed), pix, np.full(pix.shape, samp, dtype=np.uint64))
    k0, k1 = keys[:, 0].astype(np.uint64), keys[:, 1].astype(np.uint64)
    d = [((ctr_draw(k0, k1, c) >> 8).astype(f32) * f32(1.0 / 16777216.0)).astype(f32).reshape(rows, nx) for c in (0, 1)]
    return d[0], d[1]


def weights(jx, jy, dx, dy, table, radius):
    """(w, inside): the weight of a sample with the jitter (jx, jy) in the pixel (dx, dy) away, and whether it lies in the closed support"""
    R = f32(radius)
    scale = f32(TABLE) / R
    ax = np.abs((f32(dx) + jx).astype(f32) - f32(0.5)).astype(f32)
    ay = np.abs((f32(dy) + jy).astype(f32) - f32(0.5)).astype(f32)
    inside = ~(ax > R) & ~(ay > R)
    kx = np.minimum((ax * scale).astype(f32).astype(np.uint32), TABLE - 1)
    ky = np.minimum((ay * scale).astype(f32).astype(np.uint32), TABLE - 1)
    return (table[kx] * table[ky]).astype(f32), inside


def add_samples(plane, frames, i0, seed, table, radius, reach, active=None):
    """plane [rows, nx, 4] f32 += the samples frames[k] ([rows, nx, 3] f32) with the absolute indices i0 + k, in the header's order.
    active [rows, nx] bool: the pixels that are sources (None: all); every pixel is a target.  Returns the plane (changed in place)."""
    rows, nx = plane.shape[:2]
    table = np.asarray(table, dtype=f32)
    D = int(reach)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, x in enumerate(frames):
            x = np.asarray(x, dtype=f32)
            jx, jy = jitter(seed, nx, rows, i0 + k)
            for dy in range(-D, D + 1):
                tj0, tj1 = max(0, -dy), min(rows, rows - dy)
                for dx in range(-D, D + 1):
                    ti0, ti1 = max(0, -dx), min(nx, nx - dx)
                    if tj0 >= tj1 or ti0 >= ti1:
                        continue
                    src = (slice(tj0 + dy, tj1 + dy), slice(ti0 + dx, ti1 + dx))
                    w, ok = weights(jx[src], jy[src], dx, dy, table, radius)
                    if active is not None:
                        ok = ok & active[src]
                    t = plane[tj0:tj1, ti0:ti1]
                    for c in range(3):
                        t[..., c] = np.where(ok, (t[..., c] + (w * x[src][..., c]).astype(f32)).astype(f32), t[..., c])
                    t[..., 3] = np.where(ok, (t[..., 3] + w).astype(f32), t[..., 3])
    return plane


def new_plane(nx, rows):
    return np.zeros((rows, nx, 4), dtype=f32)


def read_out(plane, acc_sum, n):
    """(c [rows, nx, 3], W [rows, nx]): sum.rgb / sum.w, and where !(W > 0) the box mean acc_sum / (float)max(n, 1), n a number or the
    per-pixel counts"""
    W = plane[..., 3]
    n = np.maximum(np.broadcast_to(np.asarray(n, dtype=np.uint32), W.shape), 1).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = (plane[..., :3] / W[..., None]).astype(f32)
        box = (np.asarray(acc_sum, dtype=f32) / n[..., None]).astype(f32)
    return np.where((W > 0)[..., None], c, box).astype(f32), W.copy()


# ---- the profiles in f64, written independently of csrc/rt_filter_plan.h --------------------------------------------------------------------
def profile(kind, x, R, p0=0.0, p1=0.0):
    """f(x) of the header for 0 <= x <= R with Python floats (f64).  Box, tent and Mitchell use +, -, *, / only, in the header's order, so
    any IEEE f64 evaluation gives these bits; exp and cos may differ from another libm's in the last bit."""
    if kind == "box":
        return 1.0
    if kind == "tent":
        return 1.0 - x / R
    if kind == "gaussian":
        s2 = 2.0 * (p0 * p0)
        return math.exp(-(x * x) / s2) - math.exp(-(R * R) / s2)
    if kind == "mitchell":
        B, C, t = p0, p1, 2.0 * x / R
        if t < 1.0:
            return (((12.0 - 9.0 * B - 6.0 * C) * t + (-18.0 + 12.0 * B + 6.0 * C)) * t * t + (6.0 - 2.0 * B)) / 6.0
        return ((((-B - 6.0 * C) * t + (6.0 * B + 30.0 * C)) * t + (-12.0 * B - 48.0 * C)) * t + (8.0 * B + 24.0 * C)) / 6.0
    if kind == "blackman-harris":
        a = math.pi * x / R
        return 0.35875 + 0.48829 * math.cos(a) + 0.14128 * math.cos(2.0 * a) + 0.01168 * math.cos(3.0 * a)
    raise ValueError(kind)


def table_f64(flt, kind):
    """The 256 midpoint values of the RtPixelFilter `flt` of the named kind, f64, and each rounded once to f32"""
    R, p0, p1 = float(flt.radius), float(flt.p0), float(flt.p1)
    t64 = np.array([profile(kind, (k + 0.5) * R / TABLE, R, p0, p1) for k in range(TABLE)], dtype=np.float64)
    return t64, t64.astype(f32)


def reach_brute(R, steps=4096):
    """The largest |dq| for which some sample position dq + j - 0.5 lies within R of the centre, by a scan in f64 over draws j = k 2^-24:
    `steps` of them spread over the pixel and the 64 nearest to either edge, k = 1 .. 64 and 2^24 - 64 .. 2^24 - 1.  (The one draw j = 0,
    which touches dq = R + 0.5 exactly, has measure zero and stays outside the reach.)"""
    near = np.arange(1, 65, dtype=np.float64) * 2.0 ** -24
    j = np.concatenate([np.floor((np.arange(steps, dtype=np.float64) + 0.5) / steps * 2.0 ** 24) * 2.0 ** -24, near, 1.0 - near])
    best = 0
    for dq in range(-6, 7):
        if (np.abs(dq + j - 0.5) <= R).any():
            best = max(best, abs(dq))
    return best


def ulp_distance(a, b):
    """|a - b| in units of the last place of f32 values of one sign (or zero)"""
    ia, ib = np.asarray(a, f32).view(np.int32).astype(np.int64), np.asarray(b, f32).view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)
