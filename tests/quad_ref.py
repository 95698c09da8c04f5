"""Planar primitives (rt_set_quads, DESIGN.md "Planar primitives") in numpy float32, every operation rounded once in the kernels'
order: the set-up of (normal, D, w) and the book's quad::hit with the triangle's interior test.  The oracle knows no quads, so this
restatement is the reference of tests/test_quads.py and tests/test_quads_host.py; primary rays and the sky come from tests/lens_ref.py,
the scatter of a planar hit from tests/golden/np_ref.py (`scatter`, `Rng`, `image_value`) on the record built here."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import np_ref  # noqa: E402

f32 = np.float32
QUAD, TRIANGLE = 0, 1


def dot(a, b):
    """glam dot3 on [..., 3] float32: (ax bx + ay by) + az bz"""
    return ((a[..., 0] * b[..., 0]).astype(f32) + (a[..., 1] * b[..., 1]).astype(f32)).astype(f32) + (a[..., 2] * b[..., 2]).astype(f32)


def cross(a, b):
    return np.stack([((a[..., 1] * b[..., 2]).astype(f32) - (a[..., 2] * b[..., 1]).astype(f32)).astype(f32),
                     ((a[..., 2] * b[..., 0]).astype(f32) - (a[..., 0] * b[..., 2]).astype(f32)).astype(f32),
                     ((a[..., 0] * b[..., 1]).astype(f32) - (a[..., 1] * b[..., 0]).astype(f32)).astype(f32)], axis=-1).astype(f32)


def setup(q, u, v):
    """n = cross(u, v); normal = n / sqrt(dot(n, n)); D = dot(normal, Q); w = n / dot(n, n) — float32 [n, 3], [n], [n, 3]"""
    q, u, v = (np.asarray(x, dtype=f32).reshape(-1, 3) for x in (q, u, v))
    n = cross(u, v)
    nn = dot(n, n).astype(f32)
    normal = (n / np.sqrt(nn).astype(f32)[:, None]).astype(f32)
    D = dot(normal, q).astype(f32)
    w = (n / nn[:, None]).astype(f32)
    return normal, D, w


def hit_one(q, u, v, kind, normal, D, w, o, d, t_min, t_max):
    """quad::hit of ONE primitive for rays o, d [m, 3] (float32): (accepted [m] bool, t, alpha, beta [m] float32)"""
    o, d = np.asarray(o, dtype=f32), np.asarray(d, dtype=f32)
    with np.errstate(all="ignore"):
        denom = dot(np.broadcast_to(normal, d.shape), d).astype(f32)
        t = ((D - dot(np.broadcast_to(normal, o.shape), o).astype(f32)).astype(f32) / denom).astype(f32)
        ok = ~(np.abs(denom) < f32(1e-8)) & ~np.isnan(t) & ~(t < f32(t_min)) & ~(t > f32(t_max))
        P = (o + (d * t[:, None]).astype(f32)).astype(f32)
        p = (P - q).astype(f32)
        alpha = dot(np.broadcast_to(w, p.shape), cross(p, np.broadcast_to(v, p.shape))).astype(f32)
        beta = dot(np.broadcast_to(w, p.shape), cross(np.broadcast_to(u, p.shape), p)).astype(f32)
        if kind == TRIANGLE:
            inside = (alpha >= 0) & (beta >= 0) & ((alpha + beta).astype(f32) <= 1)
        else:
            inside = (alpha >= 0) & (alpha <= 1) & (beta >= 0) & (beta <= 1)
    return ok & inside, t, alpha, beta


def closest(q, u, v, kind, o, d, t_min=1e-3, t_max=np.finfo(f32).max, base=0, t0=None, hit0=None):
    """Closest accepted primitive per ray under the winner rule t < best || (t == best && idx > best_idx), starting from the hits
    (t0, hit0) of whatever precedes the set in the entry order.  Returns (hit index or -1, t, alpha, beta); index = base + i."""
    q, u, v = (np.asarray(x, dtype=f32).reshape(-1, 3) for x in (q, u, v))
    normal, D, w = setup(q, u, v)
    m = len(o)
    best = np.full(m, np.finfo(f32).max, f32) if t0 is None else np.asarray(t0, f32).copy()
    hit = np.full(m, -1, np.int64) if hit0 is None else np.asarray(hit0, np.int64).copy()
    al, be = np.zeros(m, f32), np.zeros(m, f32)
    for i in range(len(q)):
        ok, t, a, b = hit_one(q[i], u[i], v[i], int(kind[i]), normal[i], D[i], w[i], o, d, t_min, t_max)
        idx = base + i
        take = ok & ((t < best) | ((t == best) & (idx > hit)))
        best[take], hit[take], al[take], be[take] = t[take], idx, a[take], b[take]
    return hit, best, al, be


def hit_record(normal, o, d, t, alpha, beta):
    """The HitRecord of a planar hit for ONE ray (np_ref conventions: tuples of float32): p = o + d t, uv = (alpha, beta),
    set_face_normal(r, normal)."""
    o, d = tuple(f32(x) for x in o), tuple(f32(x) for x in d)
    on = tuple(f32(x) for x in normal)
    p = np_ref.add(o, np_ref.scale(d, f32(t)))
    front = np_ref.dot(d, on) < f32(0.0)
    return {"t": f32(t), "p": p, "on": on, "front": bool(front), "n": on if front else np_ref.neg(on), "uv": (f32(alpha), f32(beta))}


def scatter(mat, image, rec, d, key, depth):
    """Material::scatter of np_ref on a record with a uv of its own (a planar primitive's (alpha, beta), a rectangle's): a material with
    "image": True takes its colour from image_value(image, rec["uv"]).  Returns (alive, attenuation, o, d, emitted)."""
    m = dict(mat)
    if m.get("image"):
        m["tex"] = np_ref.image_value(image, rec["uv"])
    return np_ref.scatter(m, tuple(f32(x) for x in d), rec, np_ref.Rng(int(key[0]), int(key[1]), depth))
