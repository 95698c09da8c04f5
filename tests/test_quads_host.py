"""Planar primitives on the host side (no GPU): RtQuads in C and ctypes, Quad / Triangle flatten to the planar table, the two demo scenes,
and the MEASURED figure behind the culling bound of rt_set_quads (DESIGN.md "Planar primitives"): what the f32 test accepts lies within
the slack of the exact figure, and the exact figure lies inside the box the library builds."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import quad_ref

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rtquads_layout_matches_the_header(rt):
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "rtow_mi355x.h"
int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(RtQuads), offsetof(RtQuads, n), offsetof(RtQuads, q), offsetof(RtQuads, u),
    offsetof(RtQuads, v), offsetof(RtQuads, kind), offsetof(RtQuads, mat), (int)RT_PLANAR_QUAD, (int)RT_PLANAR_TRIANGLE); return 0; }'''
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "l.c"), os.path.join(td, "l")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, c], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    Q = rt._ffi.RtQuads
    assert got == [C.sizeof(Q), Q.n.offset, Q.q.offset, Q.u.offset, Q.v.offset, Q.kind.offset, Q.mat.offset, rt._ffi.PLANAR_QUAD, rt._ffi.PLANAR_TRIANGLE]


def test_abi_version_stays_11(rt):
    """the feature only adds symbols: the new entry points are in a library whose version is the one existing hosts were built against"""
    lib = rt._ffi.load_gpu_library()
    assert lib.rt_abi_version() == 11
    for name in ("rt_set_quads", "rt_multi_set_quads", "rt_debug_planar_info", "rt_debug_planar_bounds"):
        assert hasattr(lib, name), name


def test_quad_and_triangle_flatten_to_the_planar_table(rt):
    f = rt._ffi
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    red = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.8, 0.1, 0.1)))
    mirror = s.material(f.MAT_METAL, color=(0.9, 0.9, 0.9), p=(0.0,))
    s.sphere((0, 0, 0), 0.5, red, "ball")
    s.quad((1, 2, 3), (0.5, 0, 0.25), (0, 2, 0), mirror)
    a, b, c = (0.1, 0.2, 0.3), (1.7, 0.2, -0.4), (0.3, 1.9, 0.6)
    s.triangle(a, b, c, red)
    s.set_camera((0, 0, 9), (0, 0, 0), (0, 1, 0), 40.0, 1.0)
    scene = s.finish(use_bvh=False)
    q = scene.quads
    assert q.n == 2 and scene.flat.n_spheres == 1 and scene.flat.n_rects == 0
    arr = lambda p, k: np.ctypeslib.as_array(p, shape=(q.n * k,)).reshape(q.n, k) if k > 1 else np.ctypeslib.as_array(p, shape=(q.n,))
    Q, U, V, kind, mat = arr(q.q, 3), arr(q.u, 3), arr(q.v, 3), arr(q.kind, 1), arr(q.mat, 1)
    assert list(kind) == [f.PLANAR_QUAD, f.PLANAR_TRIANGLE]
    assert np.array_equal(Q[0], f32([1, 2, 3])) and np.array_equal(U[0], f32([0.5, 0, 0.25])) and np.array_equal(V[0], f32([0, 2, 0]))
    A, B, Cc = f32(a), f32(b), f32(c)
    assert np.array_equal(Q[1], A) and np.array_equal(U[1], (B - A).astype(f32)) and np.array_equal(V[1], (Cc - A).astype(f32))
    types = scene.arrays()["mat_type"]
    assert types[mat[0]] == f.MAT_METAL and types[mat[1]] == f.MAT_DIFFUSE
    # below a wrapper: refused at finish
    s2 = rt.Scene.new()
    m2 = s2.material(f.MAT_DIFFUSE, tex0=s2.constant_tex((0.5, 0.5, 0.5)))
    s2.translate(s2.quad((0, 0, 0), (1, 0, 0), (0, 1, 0), m2), (1, 0, 0))
    s2.set_camera((0, 0, 9), (0, 0, 0), (0, 1, 0), 40.0, 1.0)
    try:
        s2.finish(use_bvh=False)
        assert False, "a quad below a Translate must be refused"
    except rt.RtError:
        pass


def test_demo_scenes_build_with_the_expected_counts(rt):
    qs = rt.Scene.build("quads_scene", 1.0)
    assert qs.quads.n == 5 and qs.flat.n_spheres == 0 and qs.flat.n_rects == 0 and qs.flat.n_materials == 5
    assert set(np.ctypeslib.as_array(qs.quads.kind, shape=(5,))) == {0}
    assert np.allclose(list(qs.camera.origin), [0, 0, 9])
    ms = rt.Scene.build("mesh_scene", 16 / 9)
    n = ms.quads.n
    kind = np.ctypeslib.as_array(ms.quads.kind, shape=(n,))
    assert n == 5122 and int((kind == 1).sum()) == 5120 and int((kind == 0).sum()) == 2
    Q = np.ctypeslib.as_array(ms.quads.q, shape=(3 * n,)).reshape(n, 3)[kind == 1]
    assert np.allclose(np.linalg.norm(Q.astype(np.float64) - [0, 1, 0], axis=1), 1.0, atol=1e-6)  # vertices on the unit sphere


def _dist_to_figure(P, q, u, v, kind):
    """float64 distance of points P [m, 3] from the exact figure (q, u, v as float64)"""
    n = np.cross(u, v)
    nh = n / np.linalg.norm(n)
    h = (P - q) @ nh
    p = (P - q) - h[:, None] * nh
    G = np.array([[u @ u, u @ v], [u @ v, v @ v]])
    ab = np.linalg.solve(G, np.stack([p @ u, p @ v]))
    a, b = ab[0], ab[1]
    # closest point of the figure in the plane: brute force over the edges when outside
    if kind == quad_ref.QUAD:
        inside = (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
        edges = [(q, u), (q, v), (q + u, v), (q + v, u)]
    else:
        inside = (a >= 0) & (b >= 0) & (a + b <= 1)
        edges = [(q, u), (q, v), (q + u, v - u)]
    din = np.full(len(P), np.inf)
    for e0, ev in edges:
        s = np.clip(((p + q - e0) @ ev) / (ev @ ev), 0, 1)
        din = np.minimum(din, np.linalg.norm((p + q - e0) - s[:, None] * ev, axis=1))
    din[inside] = 0.0
    return np.sqrt(h * h + din * din)


def test_measured_bound_of_the_f32_test(rt):
    """Random quads and triangles — some at the conditioning limit sin(u, v) = 2^-10, some 1e3..1e4 units from the origin — with rays
    aimed at edges and corners from origins within RT_PLANAR_REACH W.  Asserted: (a) every hit point the f32 restatement accepts, taken in
    float64 as o + d t on the exact ray, lies within the primitive's slack of the exact figure; (b) the exact figure lies inside the box
    rt_debug_planar_bounds builds.  The largest observed distance / slack is printed (the measurement behind DESIGN.md)."""
    rng = np.random.default_rng(20261017)
    worst = 0.0
    n_acc = 0
    for case in range(160):
        far = (case % 4 == 1) * 10.0 ** rng.uniform(3, 4)
        L = 10.0 ** rng.uniform(-1, 1.5)
        q = (rng.uniform(-1, 1, 3) * max(far, 2.0)).astype(f32)
        u = (rng.normal(size=3) * L).astype(f32)
        if case % 4 == 2:  # at the conditioning limit: v nearly parallel to u
            perp = np.cross(u.astype(np.float64), rng.normal(size=3))
            perp /= np.linalg.norm(perp)
            v = (u.astype(np.float64) * rng.uniform(0.5, 2.0) + perp * np.linalg.norm(u) * 2.0 ** -10 * rng.uniform(1.05, 1.5)).astype(f32)
        else:
            v = (rng.normal(size=3) * L * rng.uniform(0.2, 2.0)).astype(f32)
        kind = case % 2
        quads = rt.make_quads(q[None], u[None], v[None], [kind], [0])
        try:
            box, slack = rt.planar_bounds(quads, 0.0)
        except rt.RtError:
            continue  # (a draw below the limit: refused, as rt_set_quads would)
        q64, u64, v64 = q.astype(np.float64), u.astype(np.float64), v.astype(np.float64)
        corners = [q64, q64 + u64, q64 + v64] + ([q64 + u64 + v64] if kind == 0 else [])
        for c in corners:  # (b)
            assert (box[0, :3] <= c).all() and (c <= box[0, 3:]).all()
        assert (box[0, 3:] - box[0, :3] >= 2 * slack[0] * (1 - 1e-6)).all()  # also the zero thickness of an axis-parallel figure
        W = max(np.abs(np.array(corners)).max(), 1e-30)
        m = 4000
        # targets: on the edges, at the corners, just inside / outside
        a, b = rng.uniform(0, 1, m), rng.uniform(0, 1, m)
        sel = rng.integers(0, 4, m)
        a[sel == 0], b[sel == 1] = 0.0, 0.0
        a[sel == 2] = 1.0 if kind == 0 else 1.0 - b[sel == 2]
        corner = rng.integers(0, 8, m) == 0
        a[corner], b[corner] = rng.integers(0, 2, corner.sum()), rng.integers(0, 2, corner.sum()) * (kind == 0)
        a += rng.normal(size=m) * 1e-6 * (rng.integers(0, 2, m))
        tgt = q64 + a[:, None] * u64 + b[:, None] * v64
        org = rng.uniform(-1, 1, (m, 3)) * rt._ffi.PLANAR_REACH * W * rng.uniform(0.01, 1.0, (m, 1))
        graze = rng.integers(0, 5, m) == 0  # nearly parallel to the plane
        nh = np.cross(u64, v64)
        nh /= np.linalg.norm(nh)
        org[graze] = tgt[graze] + (rng.normal(size=(graze.sum(), 3)) * L * 3)
        org[graze] -= ((org[graze] - tgt[graze]) @ nh)[:, None] * nh * (1 - 10.0 ** rng.uniform(-7, -2, (graze.sum(), 1)))
        d = tgt - org
        d /= np.linalg.norm(d, axis=1)[:, None]
        o32, d32 = org.astype(f32), d.astype(f32)
        normal, D, w = quad_ref.setup(q[None], u[None], v[None])
        ok, t, _, _ = quad_ref.hit_one(q, u, v, kind, normal[0], D[0], w[0], o32, d32, 1e-3, np.finfo(f32).max)
        inreach = (np.abs(o32) <= rt._ffi.PLANAR_REACH * W).all(axis=1)
        ok &= inreach
        if not ok.any():
            continue
        P = o32[ok].astype(np.float64) + d32[ok].astype(np.float64) * t[ok].astype(np.float64)[:, None]
        dist = _dist_to_figure(P, q64, u64, v64, kind)
        n_acc += int(ok.sum())
        worst = max(worst, float(dist.max() / slack[0]))
        assert dist.max() <= slack[0], (case, kind, float(dist.max()), float(slack[0]))  # (a)
    print("accepted hits: %d, largest distance / slack: %.3f" % (n_acc, worst))
    assert n_acc > 100000
