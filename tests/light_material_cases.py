"""The scenes, rays and references of tests/test_lights_materials.py (GPU) and tests/test_pbr_ref_host.py (no GPU): every material a
light set affects, at its parameter edges, below wrappers and over textures.

A ray's hit and t are the oracle's list walk without a set (a light set moves neither).  Its HitRecord is restated from the flat scene
with tests/golden/np_ref.py: sphere_hit or rect_hit below translate_hit and rotate_y_hit, composed as hitable.rs:404-520 composes
them.  Every restated record is held to the oracle before use: np_ref.scatter on it reproduces the oracle's alive, o and d bit for
bit and its attenuation to rtol 2e-5.  Then tests/light_ref.py scatters it under the set, and tests/pbr_ref64.py gives the float64 value
and the conditioning of the pbr.rs materials."""
import numpy as np

import light_ref
import pbr_ref64
import quad_ref
from helpers import path_keys

np_ref = quad_ref.np_ref
f32 = np.float32
FLT_MAX = np.finfo(f32).max
NONE = 0xFFFFFFFF
DEPTHS = (1, 7)
PBR = (6, 7, 8, 9, 10, 11, 12)
SHARP = (8, 10, 12)  # the lobes with a peak: RoughPlastic, DisneyMetal, DisneyClearcoat
CANCELLING = (9, 10, 12)  # a term that can cancel where the record faces away from the ray (see _float64)

# three sampling targets overhead: 3 x 3, a tilted one that overlaps it as seen from below, and a small one
LIGHTS = ([[-1.5, 6.0, -1.5], [-1.0, 5.0, -2.0], [1.9, 4.5, 0.9]], [[3.0, 0, 0], [2.5, 0, 0.2], [0.2, 0, 0]], [[0, 0, 3.0], [0, 0.3, 2.0], [0, 0, 0.2]])
SMALL = 2

_A, _B = (0.7, 0.5, 0.3), (0.2, 0.6, 0.9)
CASES = [
    dict(type=1, tex=(0.7, 0.3, 0.2)), dict(type=2, tex=(0.4, 0.6, 0.8)),
    dict(type=6, tex=_A, p=(0.5,)), dict(type=6, tex=_A, p=(1.0,)), dict(type=7, tex=_A, p=(0.6,)),
    dict(type=9, tex=_A, p=(0.5, 0.4)), dict(type=9, tex=_A, p=(1.0, 1.0)),
    dict(type=8, tex=_A, tex1=_B, p=(0.3, 1.5)), dict(type=8, tex=_A, tex1=_B, p=(0.01, 1.5)), dict(type=8, tex=_A, tex1=_B, p=(0.0, 1.3)),
    dict(type=8, tex=_A, tex1=_B, p=(1.0, 1.5)), dict(type=8, tex=_A, tex1=_B, p=(0.05, 1.0001)),
    dict(type=10, tex=_A, p=(0.4, 0.6, 0.125)), dict(type=10, tex=_A, p=(0.05, 0.0, 0.0)), dict(type=10, tex=_A, p=(0.0, 0.0, 0.0)),
    dict(type=10, tex=_A, p=(1.0, 1.0, 0.5)), dict(type=10, tex=_A, p=(0.3, -20.0, 0.0)), dict(type=10, tex=_A, p=(0.0, -20.0, 0.0)),
    dict(type=11, tex=_A, p=(0.0,)), dict(type=11, tex=_A, p=(0.5,)), dict(type=11, tex=_A, p=(1.0,)), dict(type=11, tex=(0.0, 0.0, 0.0), p=(0.5,)),
    dict(type=12, p=(0.0,)), dict(type=12, p=(0.7,)), dict(type=12, p=(1.0,)),
]
ONE_PER_TAG = [0, 1, 2, 4, 5, 7, 12, 19, 23]  # Diffuse, Lambert, then tags 6 to 12


def _material(s, c, tex0=None, tex1=None):
    t0 = tex0 if tex0 is not None else s.constant_tex(c["tex"]) if "tex" in c else 0xFFFFFFFF
    t1 = tex1 if tex1 is not None else s.constant_tex(c["tex1"]) if "tex1" in c else 0xFFFFFFFF
    return s.material(c["type"], tex0=t0, tex1=t1, p=c.get("p", ()))


def _begin(rt):
    s = rt.Scene.new()
    s.set_sky(rt._ffi.SKY_GRADIENT)
    s.sphere((0.0, -1000.0, 0.0), 1000.0, s.material(rt._ffi.MAT_METAL, color=(0.8, 0.7, 0.6), p=(0.1,)), "ground")
    return s


def _end(s):
    s.set_camera((0.0, 6.0, 14.0), (0.0, 0.7, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0)
    return s.finish()


def _grid(k, n):
    side = int(np.ceil(np.sqrt(n)))
    return (1.7 * (k % side - (side - 1) / 2.0), 0.7, 1.7 * (k // side - (side - 1) / 2.0))


def edges_scene(rt):
    """(a): one bare sphere per case, r = 0.7, spacing 1.7, over a Metal ground -> (scene, targets [(centre, radius, sharp)])"""
    s = _begin(rt)
    targets = []
    for k, c in enumerate(CASES):
        centre = _grid(k, len(CASES))
        s.sphere(centre, 0.7, _material(s, c), "case%d" % k)
        targets.append((centre, 0.7, c["type"] in SHARP))
    return _end(s), targets


def wrapped_scene(rt):
    """(b): one case per tag on a sphere below Translate(RotateY(..)), and on a box below the same pair for every tag but DisneyMetal
    (whose tangent a rectangle does not set)"""
    s = _begin(rt)
    targets = []
    cases = [CASES[i] for i in ONE_PER_TAG]
    boxes = [c for c in cases if c["type"] != 10]
    n = len(cases) + len(boxes)
    for k, c in enumerate(cases):
        x, y, z = _grid(k, n)
        s.translate(s.rotate_y(s.sphere((0.2, 0.0, -0.1), 0.7, _material(s, c), "wrapped%d" % k), 20.0 + 35.0 * k), (x, y, z))
        th = np.radians(20.0 + 35.0 * k)
        targets.append(((x + np.cos(th) * 0.2 + np.sin(th) * -0.1, y, z - np.sin(th) * 0.2 + np.cos(th) * -0.1), 0.7, c["type"] in SHARP))
    for k, c in enumerate(boxes):
        x, y, z = _grid(len(cases) + k, n)
        s.translate(s.rotate_y(s.gbox((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5), _material(s, c)), 15.0 + 25.0 * k), (x, 0.0, z))
        targets.append(((x, 0.5, z), 0.5, False))
    return _end(s), targets


_CHAIN4 = (("t", (0.3, 0.0, 0.0)), ("t", (0.0, 0.2, 0.0)), ("r", 30.0), ("t", (0.0, 0.0, 0.5)))  # a Translate to the object's place closes each
_CHAIN5 = (("t", (0.2, 0.0, 0.0)), ("r", -20.0), ("t", (0.0, 0.3, 0.0)), ("t", (-0.3, 0.0, 0.2)), ("r", 35.0))


def nested_scene(rt):
    """(b): spheres below five wrappers and boxes below six, each chain closed by a Translate to its place: the NEST loop"""
    s = _begin(rt)
    targets = []
    spheres = [CASES[i] for i in (0, 7, 12, 14, 23)]  # Diffuse, RoughPlastic, DisneyMetal (two), DisneyClearcoat
    boxes = [CASES[i] for i in (1, 8, 19)]             # Lambert, RoughPlastic, DisneySheen
    n = len(spheres) + len(boxes)

    def wrap(h, chain, place):
        """-> where the object-space origin lands in the world"""
        at = np.zeros(3)
        for kind, arg in chain + (("t", place),):
            if kind == "t":
                h, at = s.translate(h, arg), at + np.array(arg)
            else:
                th = np.radians(arg)
                h, at = s.rotate_y(h, arg), np.array([np.cos(th) * at[0] + np.sin(th) * at[2], at[1], -np.sin(th) * at[0] + np.cos(th) * at[2]])
        return at
    for k, c in enumerate(spheres):
        x, _, z = _grid(k, n)
        at = wrap(s.sphere((0.0, 0.0, 0.0), 0.7, _material(s, c), "deep%d" % k), _CHAIN4, (x, 0.7, z))
        targets.append((tuple(at), 0.7, c["type"] in SHARP))
    for k, c in enumerate(boxes):
        x, _, z = _grid(len(spheres) + k, n)
        at = wrap(s.gbox((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), _material(s, c)), _CHAIN5, (x, 0.4, z))
        targets.append((tuple(at), 0.5, False))
    return _end(s), targets


TEXTURED = [(0, "checker"), (0, "perlin"), (0, "image"), (1, "checker"), (1, "perlin"), (1, "image"), (5, "checker"), (5, "perlin"), (5, "image"),
            (7, "image1")]  # (case, texture): Diffuse, Lambert and DisneyDiffuse over each texture; RoughPlastic with an image as tex1


def textured_scene(rt, twin):
    """(c).  twin: the same geometry with every material replaced by Diffuse over the texture under test, so that the oracle's attenuation
    without a set is the texture's value at the hit"""
    s = _begin(rt)
    targets = []
    for k, (ci, kind) in enumerate(TEXTURED):
        tex = {"checker": lambda: s.checker_tex((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)), "perlin": lambda: s.perlin_tex(4.0),
               "image": lambda: s.image_tex("res/earthmap.jpg"), "image1": lambda: s.image_tex("res/earthmap.jpg")}[kind]()
        centre = _grid(k, len(TEXTURED))
        if twin:
            m = s.material(rt._ffi.MAT_DIFFUSE, tex0=tex)
        else:
            m = _material(s, CASES[ci], tex1=tex) if kind == "image1" else _material(s, CASES[ci], tex0=tex)
        s.sphere(centre, 0.7, m, "tex%d" % k)
        targets.append((centre, 0.7, False))
    return _end(s), targets


# ---- rays ---------------------------------------------------------------------------------------------------------------------------
def _from_above(rng, m):
    v = rng.normal(size=(m, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    v[:, 1] = np.abs(v[:, 1]) * 0.5 + 0.6
    return v / np.linalg.norm(v, axis=1)[:, None]


def _unit_xz(rng, m):
    phi = rng.uniform(0.0, 2.0 * np.pi, m)
    return np.stack([np.cos(phi), np.zeros(m), np.sin(phi)], axis=1)


def _perp(rng, a, up):
    """unit vectors perpendicular to a [m, 3]; up: on the side of +y, so that the surface met there faces the lights"""
    e = np.cross(a, rng.normal(size=a.shape))
    e /= np.linalg.norm(e, axis=1)[:, None]
    return np.where((e[:, 1] < 0)[:, None], -e, e) if up else e


def rays(targets, m, seed, mirror=0.35):
    """m rays: one in 24 at the ground beside the targets, the others in three groups: aimed at the targets' centres with jitter; at their
    limbs, 0.9 to 0.999 r off the axis, for grazing incidence; and "mirror" rays, which arrive at a point of a target so that reflect(d, n) there leads to a point of the small light (half of them
    at more than 75 degrees from the normal).  The mirror rays go to the sharp-lobed targets three times out of four."""
    rng = np.random.default_rng(seed)
    C = np.array([t[0] for t in targets], np.float64)
    R = np.array([t[1] for t in targets], np.float64)
    sharp = np.array([t[2] for t in targets], bool)
    n_mirror = int(m * mirror) if sharp.any() else 0
    n_ground = m // 24
    n_limb = (m - n_mirror - n_ground) // 2
    n_centre = m - n_mirror - n_ground - n_limb
    # the targets without a mirror ray of their own get more of the other two groups
    w = np.where(sharp, 1.0, 1.0 + 1.5 * mirror)
    pick = rng.choice(len(C), n_centre + n_limb, p=w / w.sum())
    v = _from_above(rng, len(pick))
    o = C[pick] + 8.0 * v
    off = np.concatenate([rng.normal(size=(n_centre, 3)) * 0.3, _perp(rng, -v[n_centre:], True) * rng.uniform(0.9, 0.999, (n_limb, 1))])
    tgt = C[pick] + off * R[pick][:, None]
    d = tgt - o
    O, D = [o], [d]
    far = np.abs(C[:, [0, 2]]).max() + 1.5  # the Metal ground beside the targets, which no set may change
    at = rng.uniform(far, far + 2.0, (n_ground, 1)) * _unit_xz(rng, n_ground)
    O.append(at + 8.0 * _from_above(rng, n_ground)), D.append(at - O[-1])
    if n_mirror:
        wm = np.where(sharp, 3.0 / sharp.sum(), 1.0 / max(1, (~sharp).sum()))
        pk = rng.choice(len(C), n_mirror, p=wm / wm.sum())
        Q, u, vv = (np.array(x[SMALL], np.float64) for x in LIGHTS)
        to = None
        nrm = np.zeros((n_mirror, 3))
        todo = np.ones(n_mirror, bool)
        for _ in range(64):  # (normals whose ray would start under the ground are drawn again)
            k = np.nonzero(todo)[0]
            if not len(k):
                break
            centre = C[pk[k]]
            Lp = Q + u * rng.uniform(0.2, 0.8, (len(k), 1)) + vv * rng.uniform(0.2, 0.8, (len(k), 1))
            w0 = Lp - (centre + np.array([0.0, 1.0, 0.0]) * R[pk[k]][:, None])  # towards the light, from about where the ray lands
            w0 /= np.linalg.norm(w0, axis=1)[:, None]
            th = np.where(rng.random(len(k)) < 0.5, rng.uniform(0.0, 75.0, len(k)), rng.uniform(75.0, 89.0, len(k)))
            e = _perp(rng, w0, False)
            nk = w0 * np.cos(np.radians(th))[:, None] + e * np.sin(np.radians(th))[:, None]
            x = centre + nk * R[pk[k]][:, None]
            wo = Lp - x
            wo /= np.linalg.norm(wo, axis=1)[:, None]
            din = wo - 2.0 * (wo * nk).sum(axis=1)[:, None] * nk  # reflect is its own inverse
            ok = ((wo * nk).sum(axis=1) > 0.01) & ((x - 8.0 * din)[:, 1] > 0.3)
            if to is None:
                to = np.zeros((n_mirror, 3))
                dd = np.zeros((n_mirror, 3))
            to[k[ok]], dd[k[ok]], nrm[k[ok]] = (x - 8.0 * din)[ok], din[ok], nk[ok]
            todo[k[ok]] = False
        assert not todo.any()
        O.append(to), D.append(dd)
    o, d = np.concatenate(O), np.concatenate(D)
    d /= np.linalg.norm(d, axis=1)[:, None]
    return o.astype(f32), d.astype(f32)


# ---- records ------------------------------------------------------------------------------------------------------------------------
def record(a, ns, i, o, d):
    """the HitRecord of flat primitive i (spheres, then rectangles) for the ray (o, d), through its chain of wrappers"""
    if i < ns:
        c, r = np_ref.v3(a["sph_cx"][i], a["sph_cy"][i], a["sph_cz"][i]), f32(a["sph_r"][i])
        hit = lambda ro, rd, t0, t1: np_ref.sphere_hit(c, r, ro, rd, t0, t1)
        x = int(a["sph_xform"][i]) if len(a["sph_xform"]) else NONE
    else:
        k = i - ns
        axis, mn, mx = int(a["rect_axis"][k]), np_ref.v3(*a["rect_min"][3 * k:3 * k + 3]), np_ref.v3(*a["rect_max"][3 * k:3 * k + 3])
        hit = lambda ro, rd, t0, t1: np_ref.rect_hit(axis, mn, mx, ro, rd, t0, t1)
        x = int(a["rect_xform"][k]) if len(a["rect_xform"]) else NONE
    depth = 0
    while x != NONE:  # from the innermost wrapper out
        q = tuple(f32(v) for v in a["xf_param"][4 * x:4 * x + 4])
        if int(a["xf_type"][x]) == 0:
            hit = (lambda inner, off: lambda ro, rd, t0, t1: np_ref.translate_hit(off, inner, ro, rd, t0, t1))(hit, q[:3])
        else:
            hit = (lambda inner, s_, c_: lambda ro, rd, t0, t1: np_ref.rotate_y_hit(s_, c_, inner, ro, rd, t0, t1))(hit, q[0], q[1])
        x, depth = int(a["xf_parent"][x]), depth + 1
    with np.errstate(all="ignore"):
        return hit(o, d, f32(1e-3), f32(FLT_MAX)), depth


def _mat_dict(a, j, tex=None, tex1=None):
    m = {"type": int(a["mat_type"][j]), "color": tuple(a["mat_color"][3 * j:3 * j + 3]), "p0": a["mat_p0"][j], "p1": a["mat_p1"][j], "p2": a["mat_p2"][j]}
    for key, t, given in (("tex", int(a["mat_tex0"][j]), tex), ("tex1", int(a["mat_tex1"][j]), tex1)):
        if given is not None:
            m[key] = tuple(given)
        elif t != NONE:
            assert int(a["tex_type"][t]) == 0, "a texture that is not constant needs its value from the twin scene"
            m[key] = tuple(a["tex_color0"][3 * t:3 * t + 3])
    return m


def expected(orc, scene, o, d, keys, depth, L, tex_of=None):
    """Every ray of one call: the reference under the set L.  tex_of: None, or (values [m, 3], which [n_materials] of None / "tex" / "tex1"):
    the value of a material's texture at the hit, from the twin scene.  -> dict of want (hit, t, alive, o, d, attenuation), mat (material
    index, -1 a miss), type, chain (wrappers above the primitive), rect (a rectangle), branch (0 none, 1 own, 2 light), live, wgt, below (a
    light-chosen direction below the horizon), dead and dead_att (an affected ray that ends, and the colour it is left with), p_L, n_contrib, of the family's live rays n, on, rd, dir_o and A32 (before the weight), and what
    _float64 adds."""
    a = scene.arrays()
    ns, n_prims = scene.flat.n_spheres, scene.flat.n_spheres + scene.flat.n_rects
    m = len(o)
    static = orc.debug_bounce(scene.flat_ptr, o, d, keys, depth=depth, accel=orc.ACCEL_LIST)
    want = {k: static[k].copy() for k in ("hit", "t", "alive", "o", "d", "attenuation")}
    X = dict(want=want, static=static, mat=np.full(m, -1), type=np.full(m, -1), chain=np.zeros(m, int), rect=np.zeros(m, bool), branch=np.zeros(m, int),
             wgt=np.zeros(m, f32), below=np.zeros(m, bool), p_L=np.zeros(m, f32), n_contrib=np.zeros(m, int), n=np.zeros((m, 3), f32), on=np.zeros((m, 3), f32),
             rd=d.copy(), dir_o=np.zeros((m, 3), f32), A32=np.zeros((m, 3), f32), dead_att=np.zeros((m, 3), f32), tex=np.zeros((m, 3), f32), tex1=np.zeros((m, 3), f32))
    mats = np.concatenate([a["sph_mat"], a["rect_mat"]]).astype(np.int64)
    bits = lambda v: np.array(v, f32).view(np.uint32)
    for k in range(m):
        h = int(static["hit"][k])
        if h < 0:
            continue
        assert h < n_prims
        j = int(mats[h])
        ty = int(a["mat_type"][j])
        X["mat"][k], X["type"][k], X["rect"][k] = j, ty, h >= ns
        if ty not in light_ref.AFFECTED:
            continue
        ok, dk = tuple(f32(x) for x in o[k]), tuple(f32(x) for x in d[k])
        rec, X["chain"][k] = record(a, ns, h, ok, dk)
        assert rec is not None and bits(rec["t"]) == bits(static["t"][k]), ("the oracle's t", k, h)
        given = {}
        if tex_of is not None and tex_of[1][j] is not None:
            given[tex_of[1][j]] = tex_of[0][k]
        mm = _mat_dict(a, j, **given)
        rng = lambda: np_ref.Rng(int(keys[k][0]), int(keys[k][1]), depth)
        with np.errstate(all="ignore"):
            # without a set the restatement is the oracle's own answer: the record and the material are the right ones
            al0, att0, so0, sd0, _ = np_ref.scatter(mm, dk, rec, rng())
            assert bool(al0) == bool(static["alive"][k]) and np.array_equal(bits(so0), bits(static["o"][k])) and np.array_equal(bits(sd0), bits(static["d"][k])), (k, h, mm)
            assert np.allclose(np.array(att0, f32), static["attenuation"][k], rtol=2e-5, atol=0, equal_nan=True), (k, h, mm, att0, static["attenuation"][k])
            alive, att, so, sd, _, info = light_ref.scatter(mm, dk, rec, rng(), L)
        X["branch"][k] = 1 if info["branch"] == "own" else 2
        X["below"][k] = info["branch"] == "light" and not alive
        want["alive"][k] = 1 if alive else 0
        want["o"][k], want["d"][k], want["attenuation"][k] = (so, sd, att) if alive else (0, 0, 0)
        if not alive:
            X["dead_att"][k] = att  # (what scatter leaves in the attenuation of a path it ends: 1, material.rs:12-14)
        if alive:
            X["wgt"][k], X["p_L"][k], X["n_contrib"][k] = info["wgt"], info["p_L"], info["n_contrib"]
            X["n"][k], X["on"][k], X["dir_o"][k], X["A32"][k] = rec["n"], rec["on"], sd, info["att"]
            X["tex"][k], X["tex1"][k] = mm.get("tex", (0, 0, 0)), mm.get("tex1", (0, 0, 0))
    X["live"] = (X["branch"] > 0) & (want["alive"] == 1)
    X["dead"] = (X["branch"] > 0) & (want["alive"] == 0)
    X["a"] = a
    _float64(X)
    return X


def _float64(X):
    """A64 [m, 3] and S [m] of the live rays on the pbr.rs materials (tests/pbr_ref64.py), material by material; n_dot_h of every live
    family ray; and their classes: inverted, unheld, well- and ill-conditioned"""
    a, m = X["a"], len(X["mat"])
    X["A64"], X["S"] = np.zeros((m, 3)), np.zeros(m)
    for j in np.unique(X["mat"][X["live"] & np.isin(X["type"], PBR)]):
        sel = X["live"] & (X["mat"] == j)
        args = (int(a["mat_type"][j]), X["tex"][sel], X["tex1"][sel], a["mat_p0"][j], a["mat_p1"][j], a["mat_p2"][j], X["n"][sel], X["on"][sel], X["rd"][sel], X["dir_o"][sel])
        X["A64"][sel] = pbr_ref64.attenuation(*args)
        X["S"][sel] = pbr_ref64.sensitivity(*args, seed=int(j))
    with np.errstate(all="ignore"):
        h = X["dir_o"].astype(np.float64) - X["rd"].astype(np.float64)
        h /= np.linalg.norm(h, axis=1)[:, None]
        X["n_dot_h"] = np.where(X["live"], (h * X["n"]).sum(axis=1), 0.0)
    # RotateY::hit tests the face with the inner-space direction against the outer-space normal (hitable.rs:505), so below a rotation a
    # record can face away from the ray that made it: n_dot_i <= 0.  The kernels reproduce that, and such a ray is held like any other.
    # Three BRDFs hold a term that can cancel there in binary32 however well the inputs are conditioned: 1 / (n_dot_i + n_dot_o) of
    # DisneyDiffuse, and n_dot_v + sqrt(.. + n_dot_v n_dot_v) of the Smith terms of DisneyMetal and DisneyClearcoat (at alpha_min the
    # sum is 0 and the colour infinite).  Where it does, the binary32 restatement itself leaves the rule around the float64 value, and
    # the rule cannot hold a kernel there: exactly those rays are `unheld`, decided ray by ray on the two references alone.
    # check_coverage asserts how few they are; their hit, t, alive, o and d are held bit for bit all the same.
    X["inverted"] = X["live"] & ~((X["n"].astype(np.float64) * -X["rd"].astype(np.float64)).sum(axis=1) > 0.0)
    with np.errstate(all="ignore"):
        a32, a64 = X["A32"].astype(np.float64), X["A64"]
        err = np.where(a32 == a64, 0.0, np.abs(a32 - a64))
        allowed = np.where(X["S"] <= pbr_ref64.S_WELL, 2e-5, pbr_ref64.F_REF * X["S"])[:, None] * np.abs(a64)
        meets = np.isfinite(a32).all(axis=1) & np.isfinite(a64).all(axis=1) & (err <= allowed).all(axis=1)
    X["unheld"] = X["inverted"] & np.isin(X["type"], CANCELLING) & ~meets
    pbr = X["live"] & np.isin(X["type"], PBR) & ~X["unheld"]
    X["ill"] = pbr & ~(X["S"] <= pbr_ref64.S_WELL)
    X["well"] = pbr & (X["S"] <= pbr_ref64.S_WELL)


_CACHE = {}


def reference(rt, orc, which):
    """The scene `which` ("edges", "wrapped", "nested", "textured"), its rays and its reference, computed once per process:
    dict(scene, L, per_depth=[dict(o, d, keys, depth, **expected(..))])."""
    if which in _CACHE:
        return _CACHE[which]
    build, m, seed = {"edges": (edges_scene, 6144, 5000), "wrapped": (wrapped_scene, 3072, 7000), "nested": (nested_scene, 1536, 6000),
                      "textured": (lambda r: textured_scene(r, False), 1280, 8000)}[which]
    scene, targets = build(rt)
    L = light_ref.setup(*LIGHTS)
    per_depth = []
    for depth in DEPTHS:
        o, d = rays(targets, m, seed + depth, mirror=0.35 if which == "edges" else 0.2 if which != "textured" else 0.0)
        keys = path_keys(0, np.arange(m), np.zeros(m, np.int64))  # (the production path derives slot i's key: seed 0, pixel i, sample 0)
        tex_of = None
        if which == "textured":
            twin, _ = textured_scene(rt, True)
            values = orc.debug_bounce(twin.flat_ptr, o, d, keys, depth=depth, accel=orc.ACCEL_LIST)["attenuation"]
            a = scene.arrays()
            by_mat = [None] * scene.flat.n_materials
            for k, (_, kind) in enumerate(TEXTURED):
                by_mat[int(a["sph_mat"][1 + k])] = "tex1" if kind == "image1" else "tex"
            tex_of = (values, by_mat)
        X = expected(orc, scene, o, d, keys, depth, L, tex_of)
        X.update(o=o, d=d, keys=keys, depth=depth)
        per_depth.append(X)
    _CACHE[which] = dict(scene=scene, L=L, per_depth=per_depth)
    return _CACHE[which]


def by_case(R):
    """the rays of a reference joined over its depths, for the coverage conditions: dict of arrays"""
    keys = ("mat", "type", "chain", "rect", "branch", "live", "below", "p_L", "n_contrib", "S", "ill", "well", "inverted", "unheld", "dead", "n_dot_h", "A32", "A64")
    return {k: np.concatenate([X[k] for X in R["per_depth"]]) for k in keys}


# ---- what keeps a test from passing emptily, on the references alone ------------------------------------------------------------------
def check_coverage(which, R):
    B = by_case(R)
    a = R["per_depth"][0]["a"]
    live, fam = B["live"], B["branch"] > 0
    assert B["below"].any(), "a light-chosen direction below the horizon"
    assert ((B["branch"] == 1) & live & (B["p_L"] > 0)).any(), "an own direction with p_L > 0"
    assert (B["n_contrib"] >= 2).any(), "two lights contribute to p_L"
    for j in np.unique(B["mat"][fam]):
        ty, of = int(a["mat_type"][j]), live & (B["mat"] == j)
        own, light = int((of & (B["branch"] == 1)).sum()), int((of & (B["branch"] == 2)).sum())
        if which == "edges":
            assert own >= 150 and light >= 150, (which, j, ty, own, light)
            if ty in SHARP:
                assert int((of & ~B["unheld"] & (B["n_dot_h"] >= 0.999)).sum()) >= 20, (which, j, ty, "rays on the peak")
        else:
            assert own + light >= 100 and own >= 30 and light >= 30, (which, j, ty, own, light)
        depth = np.unique(B["chain"][of])
        assert len(depth) == 1 and {"edges": depth[0] == 0, "textured": depth[0] == 0, "wrapped": depth[0] == 2, "nested": depth[0] in (5, 6)}[which], (which, j, depth)
        if ty in PBR:  # the caps of the conditioning rule: it may not swallow a case, and a bound must be a number
            ill, well, unheld = int((of & B["ill"]).sum()), int((of & B["well"]).sum()), int((of & B["unheld"]).sum())
            assert np.isfinite(B["S"][of & (B["ill"] | B["well"])]).all(), (which, j, ty, "S")
            assert 2 * ill <= own + light and well >= (150 if which != "textured" else 100), (which, j, ty, ill, well, own + light)
            assert 20 * unheld <= own + light, (which, j, ty, unheld, own + light)  # at most one ray in 20 of a case without a colour rule
    assert not B["unheld"].any() or which in ("wrapped", "nested"), which  # (no rotation, no record that faces away)
    types = set(int(t) for t in B["type"][live & fam])
    if which in ("edges", "wrapped"):
        assert types == set(light_ref.AFFECTED), types
    if which == "wrapped":
        assert set(int(t) for t in B["type"][live & fam & B["rect"]]) == set(light_ref.AFFECTED) - {10}
    if which == "nested":
        assert 10 in types and B["rect"][live & fam].any() and not B["rect"][live & fam].all()
