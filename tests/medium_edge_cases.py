"""The scenes and ray classes of tests/test_medium_edges.py (GPU) and tests/test_medium_ref_host.py (no GPU): ConstantMedium::hit where it
can go wrong.  Every class names the edge it aims at.  A class is one scene, built twice — with its media, and without them for the
closest SOLID hit and its scatter record (the oracle's list walk over the twin; tests/medium_ref.py) — and one or more calls of a few
thousand rays at most.  The key of ray i is the one the production kernels derive for slot i, path_keys(0, i, 0): a class that needs a
certain draw chooses which ray goes to which index.  Media have a constant albedo unless the class is about the albedo; solid walls
(rectangles and a sphere, Diffuse) stand among the media of every scene.

Classes:
  densities   1e-4, 1e-2, 1, 1e3, 1e6 on a box and on a sphere: from almost never scattering to scattering within an ulp of the entry
  draws       xi = 0 (never scatters), 2^-24 and 1 - 2^-24 on chosen slots (tests/golden/medium_draw_keys.json), every other slot a spread
  window      the second search's t_min = t1 + 0.0001: slabs whose thickness along the ray, in t, sweeps a quarter ulp at a time across 1e-4
              for directions of length 1e-3, 1 and 1e3; rays cutting a box corner with t2 - t1 around 1e-4; sphere rays with a negative,
              zero and tiny discriminant
  far_entry   entries on both sides of 1024 and 2048, where fl(t1 + 0.0001) is t1 + 1 ulp and then t1 itself (the second search finds the
              first root again: no scatter): origins outside (t1 > 0) and inside (t1 < 0), boxes and spheres, the r = 5000 mist of
              final_scene among them
  origins     inside the boundary; on a face plane with the direction in it (0/0, see medium_ref: nan_plane); on an edge; on a corner; on
              the sphere's surface; outside looking away (t2 < t_min)
  ties        a wall within -3 .. +3 ulp of the scatter point (the direction tuned ray by ray on the reference's own arithmetic); a smoke
              box on a floor seen from above (the floor at the exit t2) and from below (at the entry t1), a very dense one among them;
              two overlapping media whose scatter points lie within a few ulp of each other
  wrapped_*   the same box and sphere below Translate(RotateY(..)) as one common chain; wrappers AROUND the medium (ray_len is the rotated
              ray's); both at once; and boundaries the one-evaluation path does not take: two boxes as one boundary (12 rectangles), bare
              and with the second below a chain of its own (the flat scene is retagged: the host API has no list boundary)
  textured    a Perlin and a checker albedo: the colour at the outcome's own p"""
import ctypes as C
import json
import os

import numpy as np

import medium_ref as mr
from helpers import path_keys

f32 = np.float32
ALBEDO = (0.73, 0.61, 0.42)
CLASSES = ("densities", "draws", "window", "far_entry", "origins", "ties", "wrapped_common", "wrapped_around", "wrapped_both", "wrapped_slow",
           "wrapped_mixed", "textured")
DENSITIES = (1e-4, 1e-2, 1.0, 1e3, 1e6)
TIE_STEPS = (0, -1, 0, 0, -1, 1, 0, -1, 0, 2, -2, 0, 3, -3, 0, -1)  # wall t minus scatter t, in ulp, that the tuned rays of `ties` aim at

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "medium_draw_keys.json")) as _f:
    DRAW_KEYS = json.load(_f)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sphere_dirs(rng, n):
    return _unit(rng.normal(size=(n, 3)))


class Retagged:
    """A finished scene whose flat description is changed after the fact: the rectangles of its LAST medium become part of the boundary of
    the one before, and the last medium goes.  It offers what the tests use of a Scene (flat, flat_ptr, arrays, camera)."""

    def __init__(self, rt, scene):
        self._scene, self._rt = scene, rt
        fs = scene.flat
        self._flat = type(fs)()
        C.memmove(C.byref(self._flat), C.byref(fs), C.sizeof(fs))
        tag = np.ctypeslib.as_array(fs.rect_medium, shape=(fs.n_rects,)).astype(np.uint32, copy=True)
        assert fs.n_media >= 2 and (tag == fs.n_media - 1).sum() == 6
        tag[tag == fs.n_media - 1] = fs.n_media - 2
        self._tag = tag
        self._flat.rect_medium = tag.ctypes.data_as(type(fs.rect_medium))
        self._flat.n_media = fs.n_media - 1

    flat = property(lambda self: self._flat)
    flat_ptr = property(lambda self: C.pointer(self._flat))
    camera = property(lambda self: self._scene.camera)

    def arrays(self):
        return self._rt.Scene.arrays(self)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
class _Builder:
    def __init__(self, rt, media):
        f = rt._ffi
        self.rt, self.media, self.s = rt, media, rt.Scene.new()
        s = self.s
        s.set_sky(f.SKY_GRADIENT)
        self.wall = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.6, 0.5, 0.4)))
        self.hull = s.material(f.MAT_DIELECTRIC, p=(1.5,))  # the material of a boundary is never used

    def box(self, mn, mx):
        return lambda: self.s.gbox(tuple(mn), tuple(mx), self.hull)

    def ball(self, c, r):
        return lambda: self.s.sphere(tuple(c), r, self.hull, "hull")

    def fog(self, boundary, density, tex=None, inside=(), around=()):
        """a medium over boundary(); inside / around: wrappers (("r", degrees) or ("t", offset), innermost first) below and above it"""
        if not self.media:
            return
        s = self.s

        def wrap(h, ws):
            for w in ws:
                h = s.rotate_y(h, w[1]) if w[0] == "r" else s.translate(h, w[1])
            return h
        m = s.constant_medium(wrap(boundary(), inside), density, tex(s) if tex else s.constant_tex(ALBEDO))
        wrap(m, around)

    def walls(self, floor_y, back_z, ball, extent=40.0):
        s = self.s
        s.rect(1, (-extent, floor_y, -extent), (extent, floor_y, extent), self.wall)
        s.rect(2, (-extent, floor_y, back_z), (extent, floor_y + 30.0, back_z), self.wall)
        s.sphere(tuple(ball[:3]), ball[3], self.wall, "solid")

    def done(self, below=False):
        if below:  # from 90 below the floor, straight up at the dense box of `ties`: a primary ray meets the floor and the box's bottom at one t
            self.s.set_camera((6.0, -90.0, 0.5), (6.0, 0.0, 0.0), (0.0, 0.0, 1.0), 3.0, 1.0)
        else:
            self.s.set_camera((0.0, 3.0, 12.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0)
        return self.s.finish()


_INSIDE = (("r", 30.0), ("t", (0.5, 0.25, -0.5)))
_AROUND = (("r", -40.0), ("t", (-0.25, 0.5, 0.75)))


def _build(rt, name, media):
    b = _Builder(rt, media)
    if name == "densities":
        b.walls(-3.0, -6.0, (0.0, 0.0, 4.0, 0.8))
        for k, dens in enumerate(DENSITIES):
            x = 6.0 * k - 12.0
            b.fog(b.box((x - 1, -1, -1), (x + 1, 1, 1)), dens)
            b.fog(b.ball((x, 0.0, 8.0), 1.0), dens)
    elif name == "draws":
        b.walls(-3.0, -6.0, (0.0, 0.0, 4.0, 0.8))
        for k in range(4):
            x = 6.0 * k - 9.0
            b.fog(b.box((x - 1, -1, -1), (x + 1, 1, 1)), 0.5)
            b.fog(b.ball((x, 0.0, 8.0), 1.0), 0.5)
    elif name == "window":
        b.walls(-9.0, -8.0, (50.0, 3.0, -3.0, 1.0), extent=150.0)
        b.fog(b.box((-5, -5, 0), (5, 5, 1e-4)), 1e4)      # |d| = 1
        b.fog(b.box((15, -5, 0), (25, 5, 0.1)), 10.0)     # |d| = 1e3
        b.fog(b.box((35, -5, 0), (45, 5, 1e-7)), 1e7)     # |d| = 1e-3
        b.fog(b.box((59, -1, -1), (61, 1, 1)), 1e4)       # corner cuts
        b.fog(b.ball((0.0, 0.0, 50.0), 0.01), 1e4)        # tangents, |d| = 1 (x = 0: the impact parameter is o.x, to the last bit)
        b.fog(b.ball((0.0, 20.0, 50.0), 1.0), 1e3)        # tangents, |d| = 1e3
    elif name == "far_entry":
        b.s.rect(2, (-2, -2, -4), (2, 2, -4), b.wall)
        b.s.sphere((0.0, -1500.0, 0.0), 300.0, b.wall, "solid")  # (large: |oc|^2 - r^2 of a small sphere cancels at these distances, and a tree may cull such a root)
        b.fog(b.ball((0.0, 0.0, 0.0), 5000.0), 1e-4)      # the mist of final_scene
        b.fog(b.box((-1, -1, -1), (1, 1, 1)), 0.5)
        b.fog(b.ball((0.0, 10.0, 0.0), 1.0), 0.5)
        b.fog(b.box((-2500, -2500, -2500), (2500, 2500, 2500)), 2e-4)
    elif name == "origins":
        b.walls(-4.0, -7.0, (3.0, 0.0, -3.0, 0.7))
        b.fog(b.box((-1, -1, -1), (1, 1, 1)), 1.0)
        b.fog(b.ball((6.0, 0.0, 0.0), 1.0), 1.0)
    elif name == "ties":
        b.s.rect(1, (-20, 0, -20), (20, 0, 20), b.wall)                 # the floor the boxes stand on
        b.s.rect(2, (-3, 0, 0.95), (3, 3, 0.95), b.wall)                # the wall through the smoke
        b.s.sphere((-6.0, 1.0, 0.0), 1.0, b.wall, "solid")
        b.fog(b.box((-1, 0, -1), (1, 2, 1)), 1.0)                       # 0: the smoke box
        b.fog(b.box((5, 0, -1), (7, 2, 1)), 1e6)                        # 1: a very dense box on the floor
        b.fog(b.box((-1, 0, 9), (1, 2, 11)), 1.0)                       # 2, 3: a box and a sphere that overlap
        b.fog(b.ball((0.5, 1.0, 10.0), 1.0), 1.0)
    elif name.startswith("wrapped_"):
        b.walls(-4.0, -9.0, (3.0, 0.0, -3.0, 0.7))
        form = name[8:]
        if form in ("common", "around", "both"):
            ins = _INSIDE if form in ("common", "both") else ()
            aro = _AROUND if form in ("around", "both") else ()
            b.fog(b.box((-1, -1, -1), (1, 1, 1)), 0.7, inside=ins, around=aro)
            b.fog(b.ball((5.0, 0.0, 0.0), 1.0), 0.7, inside=ins, around=aro)
        else:  # two boxes that become ONE boundary (Retagged): below one chain, or the second below a chain of its own
            b.fog(b.ball((5.0, 0.0, 0.0), 1.0), 0.7)
            b.fog(b.box((-1, -1, -1), (0.5, 1, 1)), 0.7)
            b.fog(b.box((0, -0.5, -0.5), (1.5, 0.5, 1.5)), 0.7, inside=() if form == "slow" else _INSIDE)
    elif name == "textured":
        b.walls(-3.0, -6.0, (0.0, 0.0, 4.0, 0.8))
        b.fog(b.box((-4, -1, -1), (-2, 1, 1)), 1.0, tex=lambda s: s.perlin_tex(4.0))
        b.fog(b.ball((3.0, 0.0, 0.0), 1.0), 1.0, tex=lambda s: s.checker_tex((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))
    else:
        raise KeyError(name)
    scene = b.done(below=name == "ties")
    if media and name in ("wrapped_slow", "wrapped_mixed"):
        scene = Retagged(rt, scene)
    return scene


# ---- rays ---------------------------------------------------------------------------------------------------------------------------
def _aimed(rng, centres, radius, n_each, lo=4.0, hi=9.0, up=True):
    """n_each rays per target: from lo .. hi away, aimed at a point within `radius` of the centre -> o, d (unit), target index"""
    O, D, T = [], [], []
    for k, c in enumerate(centres):
        u = _sphere_dirs(rng, n_each)
        if up:
            u[:, 1] = np.abs(u[:, 1]) * 0.3
            u = _unit(u)
        o = np.asarray(c) + rng.uniform(lo, hi, (n_each, 1)) * u
        at = np.asarray(c) + rng.uniform(-radius, radius, (n_each, 3))
        O.append(o), D.append(_unit(at - o)), T.append(np.full(n_each, k))
    return np.concatenate(O), np.concatenate(D), np.concatenate(T)


def _call(o, d, depth, target, group):
    n = len(o)
    return dict(o=np.asarray(o, np.float64).astype(f32), d=np.asarray(d, np.float64).astype(f32), keys=path_keys(0, np.arange(n), np.zeros(n, np.int64)),
                depth=depth, target=np.asarray(target, np.int64), group=np.asarray(group))


def _rays(name, rng):
    if name == "densities":
        c = [p for k in range(5) for p in ((6.0 * k - 12.0, 0.0, 0.0), (6.0 * k - 12.0, 0.0, 8.0))]
        o, d, t = _aimed(rng, c, 0.9, 300)
        return [_call(o, d, 2, t, np.array(DENSITIES)[t // 2].astype(str))]
    if name == "draws":
        c = [p for k in range(4) for p in ((6.0 * k - 9.0, 0.0, 0.0), (6.0 * k - 9.0, 0.0, 8.0))]
        calls = []
        for value, (depth, slot, m) in sorted(DRAW_KEYS["draws"].items()):
            n = DRAW_KEYS["slots"]
            t = rng.integers(0, 8, n)
            t[slot] = m
            u = _sphere_dirs(rng, n)
            u[:, 1] = np.abs(u[:, 1]) * 0.3
            o = np.array(c)[t] + rng.uniform(4.0, 9.0, (n, 1)) * _unit(u)
            at = np.array(c)[t] + rng.uniform(-0.5, 0.5, (n, 3))
            g = np.full(n, "spread", dtype=object)
            g[slot] = "xi=" + value
            calls.append(_call(o, _unit(at - o), depth, t, g.astype(str)))
        return calls
    if name == "window":
        O, D, T, G = [], [], [], []
        j = np.arange(-300, 301)
        s = 1.0 + 1.5e-4 * j
        for m, (x0, length) in enumerate(((0.0, 1.0), (20.0, 1e3), (40.0, 1e-3))):
            n = len(j)
            O.append(np.stack([x0 + rng.uniform(-4, 4, n), rng.uniform(-4, 4, n), np.full(n, length)], axis=1))
            D.append(np.stack([np.zeros(n), np.zeros(n), -length * s], axis=1))
            T.append(np.full(n, m)), G.append(np.full(n, "slab |d|=%g" % length))
        n = 600
        ell = np.linspace(0.5e-4, 1.5e-4, n)
        u = np.array([-1.0, 0.0, 1.0]) / np.sqrt(2.0)
        p1 = np.stack([np.full(n, 61.0), rng.uniform(-0.9, 0.9, n), 1.0 - ell / np.sqrt(2.0)], axis=1)
        O.append(p1 - 3.0 * u), D.append(np.tile(u, (n, 1))), T.append(np.full(n, 3)), G.append(np.full(n, "corner"))
        for m, cy, r, length, oz, lo, hi in ((4, 0.0, 0.01, 1.0, 50.05, 1e-9, 1e-5), (5, 20.0, 1.0, 1e3, 55.0, 1e-5, 0.05)):
            k = np.arange(-40, 41)
            rr = np.float64(f32(r))
            b = np.concatenate([(f32(r).view(np.uint32) + k).astype(np.uint32).view(f32).astype(np.float64), rr - np.exp(rng.uniform(np.log(lo), np.log(hi), 300))])
            n = len(b)
            O.append(np.stack([b, np.full(n, cy), np.full(n, oz)], axis=1)), D.append(np.tile([0.0, 0.0, -length], (n, 1)))
            T.append(np.full(n, m)), G.append(np.full(n, "tangent |d|=%g" % length))
        return [_call(np.concatenate(O), np.concatenate(D), 1, np.concatenate(T), np.concatenate(G))]
    if name == "far_entry":
        O, D, T, G = [], [], [], []
        n = 250
        for m, c in ((1, (0.0, 0.0, 0.0)), (2, (0.0, 10.0, 0.0))):
            for lo, hi in ((1000.0, 1050.0), (2030.0, 2070.0)):
                u = _sphere_dirs(rng, n)
                o = np.asarray(c) + rng.uniform(lo, hi, (n, 1)) * u
                O.append(o), D.append(_unit(np.asarray(c) + rng.uniform(-0.5, 0.5, (n, 3)) - o)), T.append(np.full(n, m)), G.append(np.full(n, "outside"))
        for lo, hi in ((2900.0, 3000.0), (3950.0, 4000.0)):  # inside the mist, heading for its centre: t1 = -(5000 - rho)
            u = _sphere_dirs(rng, n)
            O.append(rng.uniform(lo, hi, (n, 1)) * u), D.append(_unit(-u + rng.normal(size=(n, 3)) * 0.002)), T.append(np.full(n, 0)), G.append(np.full(n, "inside"))
        for lo, hi in ((-500.0, -400.0), (-1500.0, -1450.0)):  # inside the large box, heading +x: t1 = -(2500 + x)
            O.append(np.stack([rng.uniform(lo, hi, n), rng.uniform(-100, 100, n), rng.uniform(-100, 100, n)], axis=1))
            D.append(_unit(np.stack([np.ones(n), rng.normal(size=n) * 0.01, rng.normal(size=n) * 0.01], axis=1))), T.append(np.full(n, 3)), G.append(np.full(n, "inside"))
        return [_call(np.concatenate(O), np.concatenate(D), 4, np.concatenate(T), np.concatenate(G))]
    if name == "origins":
        n = 250
        O, D, T, G = [], [], [], []

        def some_axis_zero(d):  # a third of the directions lies in a coordinate plane
            k = rng.integers(0, 9, len(d))
            for ax in range(3):
                d[k == ax, ax] = 0.0
            return _unit(d)
        O.append(np.concatenate([rng.uniform(-0.99, 0.99, (n // 2, 3)), np.array([6.0, 0, 0]) + _sphere_dirs(rng, n - n // 2) * rng.uniform(0, 0.99, (n - n // 2, 1))]))
        D.append(_sphere_dirs(rng, n)), T.append(np.repeat([0, 1], [n // 2, n - n // 2])), G.append(np.full(n, "inside"))
        d = _sphere_dirs(rng, n)
        d[:, 0] = 0.0
        O.append(np.stack([np.ones(n), rng.uniform(-0.99, 0.99, n), rng.uniform(-0.99, 0.99, n)], axis=1))
        D.append(_unit(d)), T.append(np.zeros(n)), G.append(np.full(n, "face 0/0"))
        O.append(np.stack([np.ones(n), np.ones(n), rng.uniform(-0.99, 0.99, n)], axis=1))
        D.append(some_axis_zero(_sphere_dirs(rng, n))), T.append(np.zeros(n)), G.append(np.full(n, "edge"))
        O.append(np.ones((n, 3))), D.append(some_axis_zero(_sphere_dirs(rng, n))), T.append(np.zeros(n)), G.append(np.full(n, "corner"))
        O.append(np.array([6.0, 0, 0]) + _sphere_dirs(rng, n)), D.append(_sphere_dirs(rng, n)), T.append(np.ones(n)), G.append(np.full(n, "sphere surface"))
        u = _sphere_dirs(rng, n)
        t = rng.integers(0, 2, n)
        O.append(np.array([[0.0, 0, 0], [6.0, 0, 0]])[t] + 3.0 * u), D.append(_unit(u + rng.normal(size=(n, 3)) * 0.2)), T.append(t), G.append(np.full(n, "looking away"))
        return [_call(np.concatenate(O), np.concatenate(D), 3, np.concatenate(T), np.concatenate(G))]
    if name.startswith("wrapped_") or name == "textured":
        return None  # aimed at the media's world-space bounds once the scene is there (_late_rays)
    raise KeyError(name)


def _late_rays(name, rng, W):
    """rays for the scenes whose media sit below wrappers: aimed at the centre of each medium's boundary, moved out through its wrappers"""
    centres = []
    for m in range(W.n_media):
        i = int(W.boundary[m][0])
        a = W.a
        if i < W.ns:
            c = (a["sph_cx"][i], a["sph_cy"][i], a["sph_cz"][i])
        else:
            k = i - W.ns
            c = tuple((a["rect_min"][3 * k:3 * k + 3] + a["rect_max"][3 * k:3 * k + 3]) * f32(0.5))
        p = tuple(np.array([x], f32) for x in c)
        for w in mr._chain(a, W.prim_xform(i)):
            p = mr._xform_point_back(a, w, p)
        centres.append(tuple(float(x[0]) for x in p))
    o, d, t = _aimed(rng, centres, 1.0, 3000 // W.n_media)
    scale = np.where(rng.random(len(o)) < 0.25, 10.0 ** rng.uniform(-3, 3, len(o)), 1.0)  # a quarter of the directions is not of unit length
    return [_call(o, d * scale[:, None], 2, t, np.full(len(o), "aimed"))]


# ---- ties: rays tuned on the reference's own arithmetic -------------------------------------------------------------------------------
def _ulps(a, b):
    """a - b in binary32 steps (both positive and finite)"""
    return mr.bits(a).astype(np.int64) - mr.bits(b).astype(np.int64)


def _central_t(W, m, o, d, keys, depth):
    return mr.medium_t_set(W, m, o, d, keys, depth)[:, mr.N_L // 2]


def _tune(o, d, axis_of, which, diff, want, width=128):
    """For every ray, among the rays whose component `axis_of` of o (which = "o") or d ("d") is moved by -width .. width - 1 binary32 steps,
    the one whose diff(o, d, rows) is closest to `want`.  diff works on stacked candidates; `rows` names each one's ray."""
    n = len(o)
    j = np.arange(-width, width)
    oo, dd = np.repeat(o, len(j), axis=0), np.repeat(d, len(j), axis=0)
    x = (oo if which == "o" else dd)
    x[:, axis_of] = (mr.bits(x[:, axis_of]).astype(np.int64) + np.tile(j, n)).astype(np.uint32).view(f32)
    got = diff(oo, dd, np.repeat(np.arange(n), len(j))).reshape(n, len(j))
    miss = np.abs(got - want[:, None]).astype(np.float64)
    miss[~np.isfinite(miss)] = 1e18
    best = (miss + 1e-3 * np.abs(j)[None, :]).argmin(axis=1)
    idx = np.arange(n) * len(j) + best
    return oo[idx], dd[idx], got[np.arange(n), best]


def _ties_rays(rng, W):
    depth, n = 5, 1536
    keys = path_keys(0, np.arange(n), np.zeros(n, np.int64))
    hd = [np.log(np.maximum(mr.medium_xi(keys, depth, m).astype(np.float64), 1e-30)) * float(W.neg_inv_density[m]) for m in range(4)]  # hit_dist
    free = np.ones(n, bool)

    def take(ok, count):
        idx = np.nonzero(ok & free)[0][:count]
        free[idx] = False
        return idx
    o, d = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    target, group, aim = np.zeros(n, np.int64), np.full(n, "", dtype=object), np.zeros(n, np.int64)
    # (c) the box and the sphere that overlap: sqrt(1 - b^2) = 1 + hit_dist_sphere - hit_dist_box puts both scatter points at one t
    q = 1.0 + hd[3] - hd[2]
    ic = take((q > 0.05) & (q < 0.98) & (hd[2] < 1.9) & (hd[3] < 1.9 * q), 300)
    bb = np.sqrt(1.0 - q[ic] ** 2)
    phi = rng.uniform(0.75 * np.pi, 1.25 * np.pi, len(ic))  # (o.x is what the tuning moves: it has to move b)
    oc = np.stack([0.5 + bb * np.cos(phi), 1.0 + bb * np.sin(phi), np.full(len(ic), 14.0)], axis=1).astype(f32)
    dc = np.tile(np.array([0.0, 0.0, -1.0], f32), (len(ic), 1))
    want = np.array(TIE_STEPS)[np.arange(len(ic)) % len(TIE_STEPS)]

    def box_minus_sphere(oo, dd, rows):
        k = keys[ic][rows]
        return _ulps(_central_t(W, 2, oo, dd, k, depth), _central_t(W, 3, oo, dd, k, depth)).astype(np.float64)
    o[ic], d[ic], _ = _tune(oc, dc, 0, "o", box_minus_sphere, want, width=512)
    target[ic], group[ic], aim[ic] = 2, "two media at one point", want
    # (a) the wall through the smoke, 0.05 behind the front face: a tilt of acos(0.05 / hit_dist) puts it where the ray scatters
    ia = take((hd[0] > 0.06) & (hd[0] < 1.4), 500)
    cos = 0.05 / hd[0][ia]
    da = np.stack([np.sqrt(1.0 - cos * cos), np.zeros(len(ia)), -cos], axis=1)
    entry = np.stack([rng.uniform(-0.95, -0.65, len(ia)), rng.uniform(0.2, 1.8, len(ia)), np.ones(len(ia))], axis=1)
    oa = (entry - 3.0 * da).astype(f32)
    want = np.array(TIE_STEPS)[np.arange(len(ia)) % len(TIE_STEPS)]
    a = W.a
    wall = 1  # rectangle 1 of the scene: the wall through the smoke
    assert int(a["rect_axis"][wall]) == 2 and W.prim_medium[W.ns + wall] == mr.NONE

    def wall_minus_scatter(oo, dd, rows):
        with np.errstate(all="ignore"):
            _, tw = mr._rect_t(2, a["rect_min"][3 * wall:3 * wall + 3], a["rect_max"][3 * wall:3 * wall + 3], mr._cols(oo), mr._cols(dd), mr.T_MIN, mr.FLT_MAX, True)
        return _ulps(tw, _central_t(W, 0, oo, dd, keys[ia][rows], depth)).astype(np.float64)
    o[ia], d[ia], _ = _tune(oa, da.astype(f32), 2, "d", wall_minus_scatter, want)
    target[ia], group[ia], aim[ia] = 0, "wall at the scatter point", want
    # (b) the floor at the exit (from above) and at the entry (from below) of the smoke box and of the dense one
    for m, cx, above, count in ((0, 0.0, True, 60), (0, 0.0, False, 30), (1, 6.0, True, 30), (1, 6.0, False, n)):
        ib = take(np.ones(n, bool), count)
        at = np.stack([cx + rng.uniform(-0.9, 0.9, len(ib)), np.full(len(ib), 2.0 if above else 0.0), rng.uniform(-0.9, 0.9, len(ib))], axis=1)
        u = _sphere_dirs(rng, len(ib))
        u[:, 1] = (np.abs(u[:, 1]) + 1.5) * (1.0 if above else -1.0)
        u = _unit(u)
        far = (70.0, 120.0) if (m == 1 and not above) else (17.0, 30.0)  # from 64 on a free path of 1e-6 |ln xi| is below half an ulp of t for nearly every draw
        o[ib], d[ib] = (at + rng.uniform(*far, (len(ib), 1)) * u).astype(f32), (-u).astype(f32)
        target[ib], group[ib] = m, "floor at the %s%s" % ("exit" if above else "entry", ", dense" if m else "")
    assert not free.any(), int(free.sum())
    c = _call(o, d, depth, target, group.astype(str))
    c["o"], c["d"], c["aim"] = o, d, aim  # (already binary32: no second rounding)
    return [c]


# ---- the reference of a class ----------------------------------------------------------------------------------------------------------
_CACHE = {}
_SEEDS = {name: 9100 + k for k, name in enumerate(CLASSES)}


def reference(rt, orc, name):
    """-> dict(name, scene, twin, W, calls=[dict(o, d, keys, depth, target, group, solid: the twin's oracle record with `hit` in this scene's
    numbering, clamp, winner: the sets for the device (nan_plane rejected), clamp_ref: the clamp set as hitable.rs has it (for the oracle),
    xi [n, n_media])]), computed once per process"""
    if name in _CACHE:
        return _CACHE[name]
    scene, twin = _build(rt, name, True), _build(rt, name, False)
    W = mr.World(scene)
    assert twin.flat.n_media == 0 and twin.flat.n_spheres + twin.flat.n_rects == len(W.solid_ids)
    rng = np.random.default_rng(_SEEDS[name])
    calls = _ties_rays(rng, W) if name == "ties" else (_rays(name, rng) or _late_rays(name, rng, W))
    for c in calls:
        s = orc.debug_bounce(twin.flat_ptr, c["o"], c["d"], c["keys"], depth=c["depth"], accel=orc.ACCEL_LIST)
        s["hit"] = np.where(s["hit"] >= 0, W.solid_ids[np.maximum(s["hit"], 0)], -1).astype(np.int32)
        c["solid"] = s
        iv = [W.interval(m, c["o"], c["d"], "rejected") for m in range(W.n_media)]
        for rule in ("clamp", "winner"):
            c[rule] = mr.outcomes(W, c["o"], c["d"], c["keys"], c["depth"], s["hit"], s["t"], rule, intervals=iv)
        if name == "origins":  # the one class with a NaN plane distance
            c["clamp_ref"] = mr.outcomes(W, c["o"], c["d"], c["keys"], c["depth"], s["hit"], s["t"], "clamp", nan_plane="reference")
        else:
            c["clamp_ref"] = c["clamp"]
        c["xi"] = np.stack([mr.medium_xi(c["keys"], c["depth"], m) for m in range(W.n_media)], axis=1)
        c["iso_d"] = mr.isotropic_direction(c["keys"], c["depth"])
    _CACHE[name] = dict(name=name, scene=scene, twin=twin, W=W, calls=calls)
    return _CACHE[name]


def uploadable(rt, scene):
    """what Renderer.upload takes: a Scene, or the flat description of a Retagged one"""
    return scene if isinstance(scene, rt.Scene) else scene.flat


def texture_colour(orc, scene, tex, p):
    """the oracle's texture value at the points p [n, 3] (texture.rs through orc_texture_value)"""
    lib = orc.load()
    out = np.zeros((len(p), 3), f32)
    uv = np.zeros(2, f32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    for k in range(len(p)):
        q, r = np.ascontiguousarray(p[k], f32), np.zeros(3, f32)
        lib.orc_texture_value(scene.flat_ptr, int(tex), fp(uv), fp(q), fp(r))
        out[k] = r
    return out


def shares(c):
    """of one call: the share of rays whose set (clamp or winner) holds more than one hit index, whose clamp and winner sets differ, that
    scatter in a medium under every choice, and that never do"""
    multi = (c["clamp"]["n_hits"] > 1) | (c["winner"]["n_hits"] > 1)
    differ = ~mr.same_sets(c["clamp"], c["winner"])
    a_medium_wins = lambda S: (S["valid"] & (S["hit"] != c["solid"]["hit"][:, None].astype(np.int64))).any(axis=1)
    some = a_medium_wins(c["clamp"]) | a_medium_wins(c["winner"])
    every = ~((c["clamp"]["valid"] & (c["clamp"]["hit"] == c["solid"]["hit"][:, None])).any(axis=1)) & ~((c["winner"]["valid"] & (c["winner"]["hit"] == c["solid"]["hit"][:, None])).any(axis=1))
    return dict(multi=multi, differ=differ, scatters=every, passes=~some)
