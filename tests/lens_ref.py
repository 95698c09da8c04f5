"""The thin-lens primary rays of rt_set_lens (DESIGN.md "Thin lens") in numpy float32, every operation rounded once in the kernels'
order (glam: dot = (xx + yy) + zz, normalize = v * (1 / len)) — what tests/test_defocus.py holds the GPU to, bit for bit.  The oracle
has no lens, so this restatement is the reference."""
import numpy as np

from helpers import ctr_draw, path_keys

f32 = np.float32
LENS_TRIPS = 126  # trips of the unit-disc rejection loop: counters 2..253, then the lens centre


def lens_vectors(cam, lens_radius):
    """LU = lens_radius H / |H|, LV = lens_radius V / |V|: double, rounded once to float32, in rt_render's operation order."""
    R = float(f32(lens_radius))
    out = []
    for vec in (cam.horizontal, cam.vertical):
        v = [float(x) for x in vec]
        n = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        out.append(np.array([R * v[k] / n for k in range(3)], dtype=f32))
    return out


def pm1(r):
    """next_pm1: 2 u - 1 of the top 24 bits of a draw, exact in float32"""
    return ((np.asarray(r, dtype=np.uint64) >> 8).astype(np.float64) * 2.0 ** -23 - 1.0).astype(f32)


def disc_draws(k0, k1):
    """random_in_unit_disk per path: (rx, ry, trips).  Trip t draws counters 2 + 2t and 3 + 2t; the first pair with
    rx^2 + ry^2 < 1 (float32) is taken; a path that never gets one takes (0, 0) with trips = 0."""
    k0, k1 = np.asarray(k0, dtype=np.uint64), np.asarray(k1, dtype=np.uint64)
    n = len(k0)
    rx, ry = np.zeros(n, f32), np.zeros(n, f32)
    trips = np.zeros(n, np.int32)
    done = np.zeros(n, bool)
    for t in range(LENS_TRIPS):
        if done.all():
            break
        x, y = pm1(ctr_draw(k0, k1, 2 + 2 * t)), pm1(ctr_draw(k0, k1, 3 + 2 * t))
        take = ~done & ((x * x).astype(f32) + (y * y).astype(f32) < f32(1.0))
        rx[take], ry[take], trips[take] = x[take], y[take], t + 1
        done |= take
    return rx, ry, trips


def lens_rays(cam, p, pix_i, pix_j, samp, lens_radius, focus_dist):
    """(origins, unit directions, keys) of the given (pixel, sample) paths: main.rs:89-94 + camera.rs:40-46, then the lens."""
    keys = path_keys(int(p.seed), pix_j.astype(np.uint64) * p.nx + pix_i.astype(np.uint64), samp.astype(np.uint64))
    k0, k1 = keys[:, 0].astype(np.uint64), keys[:, 1].astype(np.uint64)

    def draw(ctr):
        return ((ctr_draw(k0, k1, ctr) >> 8).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)
    u = ((pix_i.astype(f32) + draw(0)) / f32(p.nx)).astype(f32)
    v = ((pix_j.astype(f32) + draw(1)) / f32(p.ny)).astype(f32)
    org, H, V, llc = (np.array(list(x), dtype=f32) for x in (cam.origin, cam.horizontal, cam.vertical, cam.lower_left_corner))
    dirs = np.empty((len(u), 3), dtype=f32)
    for k in range(3):
        dirs[:, k] = (((llc[k] + (u * H[k]).astype(f32)).astype(f32) + (v * V[k]).astype(f32)).astype(f32) - org[k]).astype(f32)
    o = np.tile(org, (len(u), 1)).astype(f32)
    if f32(lens_radius) > 0:
        LU, LV = lens_vectors(cam, lens_radius)
        rx, ry, _ = disc_draws(k0, k1)
        off = np.empty_like(dirs)
        for k in range(3):
            off[:, k] = ((rx * LU[k]).astype(f32) + (ry * LV[k]).astype(f32)).astype(f32)
        o = (o + off).astype(f32)
        dirs = ((f32(focus_dist) * dirs).astype(f32) - off).astype(f32)
    len2 = (((dirs[:, 0] * dirs[:, 0]).astype(f32) + (dirs[:, 1] * dirs[:, 1]).astype(f32)).astype(f32) + (dirs[:, 2] * dirs[:, 2]).astype(f32)).astype(f32)
    inv = (f32(1.0) / np.sqrt(len2).astype(f32)).astype(f32)
    return o, (dirs * inv[:, None]).astype(f32), keys


def sky_gradient(d):
    """demo_scene.rs:28-31 on unit directions [n, 3] (tests/golden/np_ref.py sky_gradient, vectorised)"""
    t = ((d[:, 1] * f32(0.5)).astype(f32) + f32(0.5)).astype(f32)
    a, b = np.ones(3, f32), np.array([0.5, 0.7, 1.0], f32)
    return (a[None, :] + ((b - a).astype(f32)[None, :] * t[:, None]).astype(f32)).astype(f32)
