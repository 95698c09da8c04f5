"""The matrix of kernel instantiations (csrc/rt_api.hip "kernel variants"): one table of rows, each a small scene, a set (none, motion,
quads, lights, quads + lights), the debug options it needs, the placement rt_debug_scene_info must show, and the keys of k_shade,
k_intersect and k_debug_bounce it CLAIMS to launch.  tests/test_variant_matrix_host.py holds the union of the claims against the
library's tables (rt_debug_variant_tables) and the coverage conditions of every row; tests/test_variant_matrix.py runs every row on the
GPU against the reference built here and holds the context's launch ledger against the row's claims.

The reference of a ray is the oracle's list walk (orc.debug_bounce) wherever the oracle knows the feature: static scenes, and moving
spheres with every mover written where tests/motion_ref.py puts it at that ray's time.  Planar primitives come from tests/quad_ref.py
on top of the oracle's hit, and the materials a light set affects from tests/light_ref.py on the record of the bare sphere or rectangle
the oracle reports (tests/golden/np_ref.py); such rays are marked `restated`.  Scenes keep affected materials off wrapped primitives,
where this module has no record to restate with.  The wrapped and nested forms hold a box of fog (below a wrapper of its own in the
nested form); a scatter inside it is the oracle's, held to the rule of test_constant_medium_and_cornell_box.

A new flag adds rows here until test_variant_matrix_host.py passes again."""
import numpy as np

import light_ref
import motion_ref
import quad_ref
from helpers import path_keys

np_ref = quad_ref.np_ref
f32 = np.float32
FLT_MAX = np.finfo(f32).max
NONE = 0xFFFFFFFF
N_RAYS = 2048
DEPTH = 1            # single rays: any depth >= 1 (the production kernels are those of a depth >= 1)
FRAME = dict(nx=48, ny=32, spp=4, max_depth=6)
LENS = (0.1, 12.0)
SHUTTER = (0.1, 0.9)
# Keys that no sequence of public calls and debug options can launch.  A kernel that cannot be launched cannot be tested: such a key leaves its
# *_variant_exists rule in csrc/rt_api.hip (DESIGN.md "Kernel variants") instead of staying here, so the sets are empty.
UNREACHABLE = {"shade": set(), "intersect": set(), "debug_bounce": set()}

# sampling targets of the light rows: above the scene, one larger and tilted that overlaps the first as seen from below
LIGHTS = ([[-1.5, 6.0, -1.5], [-1.0, 5.0, -2.0]], [[3.0, 0, 0], [2.5, 0, 0.2]], [[0, 0, 3.0], [0, 0.3, 2.0]])
AFFECTED_TYPES = (1, 2, 6, 7, 9)  # Diffuse, Lambert, OrenNayar, BurleyDiffuse, DisneyDiffuse: what light_ref restates
PBR_TYPES = (6, 7, 9)             # colours to rtol 2e-5 (atol 0), as tests/test_lights.py holds BurleyDiffuse


def _row(name, form, sets, perlin, opts, tree_in_lds, tables_in_lds, shade, isect, grid=None):
    """`shade` / `isect`: the row's key at a depth >= 1; the frames add GEN and GEN|LENS to it.  `isect` None: a grid row, whose rays never
    reach a tabled k_intersect (depth 0 comes from the candidate lists, every other depth walks the grid).  grid: None, "flat", "deep"."""
    nest = form == "nested"
    general = form not in ("spheres", "layer", "cube") or "quads" in sets or opts.get("general_kernels") == 1
    return dict(name=name, form=form, sets=tuple(sets), perlin=perlin, opts=dict(opts), shade=frozenset(shade), isect=None if isect is None else frozenset(isect),
                grid=grid, info=dict(tree_in_lds=tree_in_lds, general_tables_in_lds=tables_in_lds, nest=int(nest), general_kernels=int(general),
                                     grid=int(grid is not None), n_planar=3 if "quads" in sets else 0))


SPH = {"grid": 1, "primary_lists": 1}  # a sphere-only scene walks its tree at every depth: no grid, no candidate lists
L2 = {"tree_placement": 1}
HBM = {"general_lds": 1}
ROWS = [
    # sphere-only scenes
    _row("spheres", "spheres", (), False, SPH, 1, 0, (), ("LDS_NODES",)),
    _row("spheres_motion_perlin", "spheres", ("motion",), True, SPH, 1, 0, ("PERLIN_LDS", "MOTION"), ("LDS_NODES", "MOTION")),
    _row("spheres_l2_lights", "spheres", ("lights",), False, {**SPH, **L2}, 0, 0, ("LIGHTS",), ("RECTS",)),
    _row("spheres_l2_motion", "spheres", ("motion",), False, {**SPH, **L2}, 0, 0, ("MOTION",), ("RECTS", "MOTION")),
    _row("grid_deep_perlin", "cube", (), True, {}, 1, 0, ("PERLIN_LDS",), None, grid="deep"),
    _row("grid_flat_perlin_lights", "layer", ("lights",), True, {}, 1, 0, ("PERLIN_LDS", "LIGHTS"), None, grid="flat"),
    _row("grid_deep_motion", "cube", ("motion",), False, {}, 1, 0, ("MOTION",), None, grid="deep"),
    _row("grid_flat_motion", "layer", ("motion",), False, {}, 1, 0, ("MOTION",), None, grid="flat"),
    # general scenes: bare rectangles, then a box below two wrappers
    _row("rects", "rects", (), False, {}, 1, 0, ("RECTS",), ("RECTS", "LDS_NODES")),
    _row("wrapped_l2_lights", "wrapped", ("lights",), False, L2, 0, 1, ("RECTS", "LIGHTS"), ("RECTS", "GLDS")),
    _row("wrapped_perlin", "wrapped", (), True, {}, 1, 1, ("PERLIN_LDS", "RECTS"), ("RECTS", "LDS_NODES", "GLDS")),
    _row("rects_motion", "rects", ("motion",), False, {}, 1, 0, ("RECTS", "MOTION"), ("RECTS", "LDS_NODES", "MOTION")),
    _row("wrapped_l2_motion_perlin", "wrapped", ("motion",), True, L2, 0, 1, ("PERLIN_LDS", "RECTS", "MOTION"), ("RECTS", "GLDS", "MOTION")),
    _row("wrapped_motion", "wrapped", ("motion",), False, {}, 1, 1, ("RECTS", "MOTION"), ("RECTS", "LDS_NODES", "GLDS", "MOTION")),
    _row("general_kernels_perlin_lights", "spheres", ("lights",), True, {**SPH, "general_kernels": 1}, 1, 0, ("PERLIN_LDS", "RECTS", "LIGHTS"), ("RECTS", "LDS_NODES")),
    # a sphere and a box below chains of five and six wrappers
    _row("nested_l2_hbm", "nested", (), False, {**L2, **HBM}, 0, 0, ("RECTS", "NEST"), ("RECTS", "NEST")),
    _row("nested_hbm_lights", "nested", ("lights",), False, HBM, 1, 0, ("RECTS", "NEST", "LIGHTS"), ("RECTS", "LDS_NODES", "NEST")),
    _row("nested_l2_perlin", "nested", (), True, L2, 0, 1, ("PERLIN_LDS", "RECTS", "NEST"), ("RECTS", "GLDS", "NEST")),
    _row("nested_perlin_lights", "nested", ("lights",), True, {}, 1, 1, ("PERLIN_LDS", "RECTS", "NEST", "LIGHTS"), ("RECTS", "LDS_NODES", "GLDS", "NEST")),
    _row("nested_l2_hbm_motion", "nested", ("motion",), False, {**L2, **HBM}, 0, 0, ("RECTS", "NEST", "MOTION"), ("RECTS", "NEST", "MOTION")),
    _row("nested_hbm_motion_perlin", "nested", ("motion",), True, HBM, 1, 0, ("PERLIN_LDS", "RECTS", "NEST", "MOTION"), ("RECTS", "LDS_NODES", "NEST", "MOTION")),
    _row("nested_l2_motion", "nested", ("motion",), False, L2, 0, 1, ("RECTS", "NEST", "MOTION"), ("RECTS", "GLDS", "NEST", "MOTION")),
    _row("nested_motion", "nested", ("motion",), False, {}, 1, 1, ("RECTS", "NEST", "MOTION"), ("RECTS", "LDS_NODES", "GLDS", "NEST", "MOTION")),
    # a planar set: over spheres alone, then over a scene with wrappers (the tables beside the tree)
    _row("quads_l2", "spheres", ("quads",), False, L2, 0, 0, ("RECTS", "NEST", "PLANAR"), ("RECTS", "NEST", "PLANAR")),
    _row("quads_lights", "spheres", ("quads", "lights"), False, {}, 1, 0, ("RECTS", "NEST", "PLANAR", "LIGHTS"), ("RECTS", "LDS_NODES", "NEST", "PLANAR")),
    _row("wrapped_l2_quads_lights_perlin", "wrapped", ("quads", "lights"), True, L2, 0, 1, ("PERLIN_LDS", "RECTS", "NEST", "PLANAR", "LIGHTS"), ("RECTS", "GLDS", "NEST", "PLANAR")),
    _row("wrapped_quads_perlin", "wrapped", ("quads",), True, {}, 1, 1, ("PERLIN_LDS", "RECTS", "NEST", "PLANAR"), ("RECTS", "LDS_NODES", "GLDS", "NEST", "PLANAR")),
]
ROW_NAMES = [r["name"] for r in ROWS]


# ---- claims -------------------------------------------------------------------------------------------------------------------------
def _ordered(rt, family, names):
    """a key as variant_tables() spells it: the library's flag names in bit order"""
    order = rt.variant_flag_names(family)
    assert set(names) <= set(order), (names, order)
    return tuple(n for n in order if n in names)


def claims(rt, row):
    """What the row launches, in the form of rt.variant_tables(): its key at a depth >= 1 (single rays through the production kernels,
    the frames' deeper bounces and materialised primaries), GEN and GEN|LENS of it (depth 0 of the frames without and with a lens), the
    two k_debug_bounce forms, the list walk of its set and, for a grid row, its grid walk."""
    f = rt._ffi
    sets = row["sets"]
    out = {"shade": {_ordered(rt, f.FAMILY_SHADE, row["shade"] | extra) for extra in (set(), {"GEN"}, {"GEN", "LENS"})}}
    out["intersect"] = set() if row["isect"] is None else {_ordered(rt, f.FAMILY_INTERSECT, row["isect"] | extra) for extra in (set(), {"GEN"}, {"GEN", "LENS"})}
    db = {"motion": "MOTION", "quads": "PLANAR", "lights": "LIGHTS"}
    key = _ordered(rt, f.FAMILY_DEBUG_BOUNCE, {db[s] for s in sets})
    out["debug_bounce"] = {("TREE_LDS" if row["info"]["tree_in_lds"] else "TREE_L2",) + key, ("BRUTE",) + key}
    out["untabled"] = {"k_intersect_list_planar" if "quads" in sets else "k_intersect_list_motion" if "motion" in sets else "k_intersect_list"}
    if row["grid"]:
        out["untabled"].add("k_intersect_grid%s<%s>" % ("_motion" if "motion" in sets else "", "true" if row["grid"] == "flat" else "false"))
    return out


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
_MOVERS = [((-1.0, 2.2, 1.0), (-0.2, 2.7, 1.4), 0.45, 0), ((1.5, 2.0, 1.0), (0.9, 2.6, 0.5), 0.4, 5), ((0.0, 1.9, 3.5), (0.8, 1.9, 3.3), 0.35, 1)]
_QUADS = [("quad", (-2.5, 0.3, 3.2), (1.6, 0.0, 0.4), (0.0, 1.5, -0.5), 0), ("triangle", (1.0, 0.2, 3.6), (2.8, 0.4, 3.2), (1.8, 2.0, 2.8), 5),
          ("quad", (-0.8, 4.2, -0.8), (1.6, 0.0, 0.0), (0.0, 0.0, 1.6), 7)]  # Diffuse, Metal, an emitter


def build(rt, row):
    """-> dict(scene, motion, quads, lights): the row's scene finished, and the sets to apply after upload (None: not in this row)"""
    f = rt._ffi
    form, sets = row["form"], row["sets"]
    lights = "lights" in sets
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    const = s.constant_tex
    mats = [s.material(f.MAT_DIFFUSE, tex0=const((0.7, 0.3, 0.2))), s.material(f.MAT_LAMBERT, tex0=const((0.4, 0.6, 0.8))),
            s.material(f.MAT_OREN_NAYAR, tex0=const((0.6, 0.6, 0.3)), p=(0.5,)), s.material(f.MAT_BURLEY_DIFFUSE, tex0=const((0.8, 0.7, 0.3)), p=(0.6,)),
            s.material(f.MAT_DISNEY_DIFFUSE, tex0=const((0.5, 0.7, 0.5)), p=(0.5, 0.4)), s.material(f.MAT_METAL, color=(0.8, 0.7, 0.6), p=(0.1,)),
            s.material(f.MAT_DIELECTRIC, p=(1.5,)), s.material(f.MAT_EMISSION, tex0=const((4.0, 4.0, 4.0)))]
    ground = s.material(f.MAT_DIFFUSE, tex0=const((0.5, 0.5, 0.5)))
    perlin = []
    if row["perlin"]:  # on an emitter (no set touches it); on a Diffuse sphere too unless a light set would change that material's samples
        perlin.append(s.material(f.MAT_EMISSION, tex0=s.perlin_tex(2.0)))
        if not lights:
            perlin.append(s.material(f.MAT_DIFFUSE, tex0=s.perlin_tex(4.0)))

    def sphere(c, r, m, name, c1=None):
        if c1 is not None and "motion" in sets:
            return s.moving_sphere(c, c1, r, m, name)
        return s.sphere(c, r, m, name)

    s.sphere((0.0, -100.0, 0.0), 100.0, ground, "ground")
    if form in ("layer", "cube"):  # 25 / 27 small spheres: enough for a uniform grid, one cell high or several
        cells = [(i, 0, k) for i in range(5) for k in range(5)] if form == "layer" else [(i, j, k) for i in range(3) for j in range(3) for k in range(3)]
        off = 2.0 if form == "layer" else 1.0
        for n, (i, j, k) in enumerate(cells):
            c = ((i - off) * 1.6, 0.3 + 1.6 * j, (k - off) * 1.6)
            m = perlin[n % len(perlin)] if perlin and n % 4 == 1 else mats[n % 7]
            # (a flat grid stays flat: its movers keep their height)
            sphere(c, 0.3, m, "g%d" % n, c1=(c[0] + 0.7, c[1] + (0.0 if form == "layer" else 0.5), c[2] + 0.4) if n % 5 == 2 else None)
    else:
        for k in range(5):  # the five materials a light set affects, on bare spheres
            s.sphere((-4.0 + 2.0 * k, 0.7, 0.0), 0.7, mats[k], "affected%d" % k)
        s.sphere((-3.0, 0.5, 2.5), 0.5, mats[5], "metal")
        s.sphere((3.0, 0.5, 2.5), 0.5, mats[6], "glass")
        for k, m in enumerate(perlin):
            s.sphere(((0.0, 3.2, -1.5), (0.0, 0.6, 2.8))[k], (0.7, 0.6)[k], m, "perlin%d" % k)
        for k, (c0, c1, r, m) in enumerate(_MOVERS):
            sphere(c0, r, mats[m], "mover%d" % k, c1=c1)
        if form in ("rects", "wrapped", "nested"):
            s.rect(f.RECT_XZ, (-1.5, 6.0, -1.5), (1.5, 6.0, 1.5), mats[7])
            s.rect(f.RECT_XY, (-5.0, 0.0, -3.5), (5.0, 4.0, -3.5), mats[1])
        if form in ("wrapped", "nested"):
            s.translate(s.rotate_y(s.gbox((0.0, 0.0, 0.0), (1.0, 1.4, 1.0), mats[5]), 25.0), (-5.8, 0.0, 1.2))
            fog = s.constant_tex((0.8, 0.85, 0.9))
            if form == "wrapped":  # a box of fog; below a wrapper of its own in the nested form (a wrapper around a medium nests)
                s.constant_medium(s.gbox((4.6, 0.0, 1.2), (6.2, 1.5, 2.8), mats[0]), 2.0, fog)
            else:
                s.translate(s.constant_medium(s.gbox((0.0, 0.0, 0.0), (1.6, 1.5, 1.6), mats[0]), 2.0, fog), (4.6, 0.0, 1.2))
        if form == "nested":
            h = s.sphere((0.0, 0.6, 0.0), 0.6, mats[5], "deep")
            for kind, arg in (("t", (1.0, 0.0, 0.0)), ("t", (0.0, 0.5, 0.0)), ("r", 30.0), ("t", (0.0, 0.0, 1.5)), ("t", (1.5, 0.6, 1.0))):
                h = s.translate(h, arg) if kind == "t" else s.rotate_y(h, arg)
            h = s.gbox((0.0, 0.0, 0.0), (0.9, 0.9, 0.9), mats[6])
            for kind, arg in (("t", (0.2, 0.0, 0.0)), ("r", -20.0), ("t", (0.0, 0.3, 0.0)), ("t", (-1.0, 0.0, 0.5)), ("r", 35.0), ("t", (-2.5, 1.2, 1.5))):
                h = s.translate(h, arg) if kind == "t" else s.rotate_y(h, arg)
    if "quads" in sets:
        for kind, a, b, c, m in _QUADS:
            (s.quad if kind == "quad" else s.triangle)(a, b, c, mats[m])
    s.set_camera((0.0, 4.0, 12.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 40.0, FRAME["nx"] / FRAME["ny"], shutter=SHUTTER if "motion" in sets else (0.0, 1.0))
    scene = s.finish()
    out = dict(scene=scene, motion=None, quads=None, lights=None)
    if "motion" in sets:
        out["motion"] = scene.motion
        assert out["motion"].n_moving >= 3
    if "quads" in sets:
        out["quads"] = scene.quads
        assert out["quads"].n == 3
    if lights:
        out["lights"] = rt.make_lights(*LIGHTS)
    return out


# ---- rays ---------------------------------------------------------------------------------------------------------------------------
def _quad_arrays(quads):
    n = quads.n
    g = lambda p, k, t: np.ctypeslib.as_array(p, shape=(n * k,)).reshape((n, k) if k > 1 else (n,)).astype(t)
    return g(quads.q, 3, f32), g(quads.u, 3, f32), g(quads.v, 3, f32), g(quads.kind, 1, np.uint8), g(quads.mat, 1, np.uint32)


def _motion_arrays(motion):
    n = motion.n_moving
    return np.ctypeslib.as_array(motion.sphere, shape=(n,)).astype(np.int64), np.ctypeslib.as_array(motion.center1, shape=(3 * n,)).reshape(n, 3).astype(f32)


def _chain_depth(a, x):
    n = 0
    while x != NONE:
        n, x = n + 1, int(a["xf_parent"][x])
    return n


def _prims(rt, B):
    """Per primitive of the flat scene (spheres, then rectangles): world centre and size for aiming, wrapper chain depth, material."""
    scene = B["scene"]
    a, fs = scene.arrays(), scene.flat
    wb = rt.world_bounds(scene)
    ns, nr = fs.n_spheres, fs.n_rects
    xf = np.concatenate([a["sph_xform"] if len(a["sph_xform"]) else np.full(ns, NONE, np.uint32), a["rect_xform"] if len(a["rect_xform"]) else np.full(nr, NONE, np.uint32)])
    box = wb["prim_box"].astype(np.float64)
    med = np.concatenate([a["sph_medium"] if len(a["sph_medium"]) else np.full(ns, NONE, np.uint32), a["rect_medium"] if len(a["rect_medium"]) else np.full(nr, NONE, np.uint32)])
    mbox = wb["entry_box_padded"][wb["entry_id"] >= ns + nr].astype(np.float64)  # the media, in index order
    return dict(a=a, ns=ns, nr=nr, boundary=med != NONE, media_centre=mbox.mean(axis=1), media_half=(mbox[:, 1] - mbox[:, 0]) / 2, centre=box.mean(axis=1), half=(box[:, 1] - box[:, 0]) / 2, chain=np.array([_chain_depth(a, int(x)) for x in xf]),
                mat=np.concatenate([a["sph_mat"], a["rect_mat"]]).astype(np.int64))


def _perlin_mats(rt, a):
    tex = a["mat_tex0"]
    return np.array([t != NONE and a["tex_type"][t] == rt._ffi.TEX_PERLIN for t in tex])


def rays(rt, row, B):
    """N_RAYS rays from a shell around the scene at its primitives (the ground gets the strays), more of them at what the row exists for:
    movers where they are in mid-shutter, the deep chains, the planar set, the Perlin spheres."""
    rng = np.random.default_rng(ROW_NAMES.index(row["name"]) + 1000)
    P = _prims(rt, B)
    perlin = _perlin_mats(rt, P["a"])
    tgt, jit, w = [], [], []
    moving = set()
    if B["motion"] is not None:
        idx, c1 = _motion_arrays(B["motion"])
        moving = set(int(i) for i in idx)
        for i, e in zip(idx, c1):
            tgt.append((P["centre"][i] + e) / 2), jit.append(P["half"][i] * 0.6), w.append(4.0 if row["grid"] is None else 1.5)
    for i in range(P["ns"] + P["nr"]):
        if i == 0 or i in moving or P["boundary"][i]:
            continue
        tgt.append(P["centre"][i]), jit.append(P["half"][i] * 0.45)
        ty, lit = int(P["a"]["mat_type"][P["mat"][i]]), "lights" in row["sets"]
        if P["chain"][i] > 0:  # (a box is six rectangles)
            w.append((2.0 if i < P["ns"] else 0.4) if P["chain"][i] > 4 else 1.2)
        elif perlin[P["mat"][i]]:
            w.append(8.0 if lit else 2.5)
        elif i >= P["ns"]:
            w.append(0.5)
        else:
            w.append((8.0 if ty in PBR_TYPES else 3.0 if ty in (1, 2) else 1.0) if lit else 1.5 if ty == 3 else 1.0)
    for c, h in zip(P["media_centre"], P["media_half"]):
        tgt.append(c), jit.append(h * 0.4), w.append(12.0 if "lights" in row["sets"] else 5.0)
    if B["quads"] is not None:
        q, u, v, kind, _ = _quad_arrays(B["quads"])
        for i in range(len(q)):
            tgt.append(q[i] + (u[i] + v[i]) * (0.5 if kind[i] == 0 else 0.3)), jit.append((np.abs(u[i]) + np.abs(v[i])) * (0.2 if kind[i] == 0 else 0.1))
            w.append(3.0 if kind[i] == 0 else 7.0)
    w = np.array(w) / np.sum(w)
    pick = rng.choice(len(tgt), N_RAYS, p=w)
    target = np.array(tgt)[pick] + rng.normal(size=(N_RAYS, 3)) * np.array(jit)[pick]
    vdir = rng.normal(size=(N_RAYS, 3))
    vdir /= np.linalg.norm(vdir, axis=1)[:, None]
    vdir[:, 1] = np.abs(vdir[:, 1]) * 0.8 + 0.05
    o = (np.array([0.0, 1.0, 0.0]) + 9.0 * vdir).astype(f32)
    d = target - o
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(f32)
    return o, d


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def _mat_dict(rt, a, j):
    """material j of the flat scene in np_ref's spelling (constant textures only: None for any other)"""
    m = {"type": int(a["mat_type"][j]), "color": tuple(a["mat_color"][3 * j:3 * j + 3]), "p0": a["mat_p0"][j], "p1": a["mat_p1"][j], "p2": a["mat_p2"][j]}
    t = int(a["mat_tex0"][j])
    if t != NONE:
        if int(a["tex_type"][t]) != rt._ffi.TEX_CONSTANT:
            return None
        m["tex"] = tuple(a["tex_color0"][3 * t:3 * t + 3])
    return m


def _centre_views(scene):
    fs = scene.flat
    return [np.ctypeslib.as_array(p, shape=(fs.n_spheres,)) for p in (fs.sph_cx, fs.sph_cy, fs.sph_cz)]


def _oracle_at(orc, scene, idx, c0, c1, tm, o, d, keys):
    """the oracle's list walk over the scene with mover idx[k] at motion_ref.center_at(c0[k], c1[k], tm) — every ray of the call at that
    one time; the scene's own centres are put back"""
    views = _centre_views(scene)
    at = np.stack([motion_ref.center_at(c0[k], c1[k], tm)[0] for k in range(len(idx))]) if len(idx) else np.zeros((0, 3), f32)
    try:
        for ax in range(3):
            views[ax][idx] = at[:, ax]
        return orc.debug_bounce(scene.flat_ptr, o, d, keys, depth=DEPTH, accel=orc.ACCEL_LIST)
    finally:
        for ax in range(3):
            views[ax][idx] = c0[:, ax]


_CACHE = {}


def _reference_motion(orc, scene, motion, centre_of, o, d, keys, want, stats):
    """every ray has its own time: the oracle on the scene as it is then, written into `want`"""
    idx, c1 = _motion_arrays(motion)
    c0 = centre_of[idx].copy()
    tm = motion_ref.path_time(keys, *SHUTTER)
    assert tm.min() >= SHUTTER[0] and tm.max() <= SHUTTER[1] and tm.std() > 0.15
    for k in range(len(o)):
        one = _oracle_at(orc, scene, idx, c0, c1, tm[k], o[k:k + 1], d[k:k + 1], keys[k:k + 1])
        for key in want:
            want[key][k] = one[key][0]
    ends = [_oracle_at(orc, scene, idx, c0, c1, f32(t), o, d, keys) for t in SHUTTER]
    stats["moved"] = int(((ends[0]["hit"] != ends[1]["hit"]) | (ends[0]["t"].view(np.uint32) != ends[1]["t"].view(np.uint32))).sum())
    stats["mover_hits"] = int(np.isin(want["hit"], idx).sum())


def _reference_quads(quads, base, o, d, want, stats):
    """the planar set on top of the hits in `want` (quad_ref's winner rule): hit and t are written into `want`;
    -> {ray: (record, flat material)} of the rays a planar primitive wins"""
    q, u, v, kind, qmat = _quad_arrays(quads)
    hit0 = want["hit"].astype(np.int64)
    t0 = np.where(hit0 >= 0, want["t"], f32(FLT_MAX)).astype(f32)
    ph, pt, al, be = quad_ref.closest(q, u, v, kind, o, d, base=base, t0=t0, hit0=hit0)
    normal, _, _ = quad_ref.setup(q, u, v)
    recs = {}
    for k in np.nonzero(ph >= base)[0]:
        i = int(ph[k]) - base
        recs[int(k)] = (quad_ref.hit_record(normal[i], o[k], d[k], pt[k], al[k], be[k]), int(qmat[i]))
        want["hit"][k], want["t"][k] = ph[k], pt[k]
    stats["quad_hits"] = sum(1 for k in recs if kind[int(ph[k]) - base] == 0)
    stats["triangle_hits"] = sum(1 for k in recs if kind[int(ph[k]) - base] == 1)
    return recs


def _bare_record(P, centre_of, i, ok, dk):
    """the HitRecord of bare primitive i (a sphere, then the rectangles) for one ray, from tests/golden/np_ref.py"""
    a, ns = P["a"], P["ns"]
    assert P["chain"][i] == 0 and not P["boundary"][i], ("a primitive this module cannot restate", i)
    if i < ns:
        return np_ref.sphere_hit(np_ref.v3(*centre_of[i]), f32(a["sph_r"][i]), ok, dk, f32(1e-3), f32(FLT_MAX))
    r = i - ns
    return np_ref.rect_hit(int(a["rect_axis"][r]), np_ref.v3(*a["rect_min"][3 * r:3 * r + 3]), np_ref.v3(*a["rect_max"][3 * r:3 * r + 3]), ok, dk, f32(1e-3), f32(FLT_MAX))


def _restate(rt, row, P, L, planar_recs, centre_of, o, d, keys, static, want):
    """The rays the oracle cannot answer: planar hits (np_ref.scatter on quad_ref's record, light_ref.scatter under a light set) and,
    under a light set, hits of an affected material on a bare primitive.  Writes them into `want`; -> (restated [n] bool, info [n])."""
    a, n, n_prims = P["a"], len(o), P["ns"] + P["nr"]
    restated, info = np.zeros(n, bool), [None] * n
    for k in range(n):
        h = int(want["hit"][k])
        ok, dk = tuple(f32(x) for x in o[k]), tuple(f32(x) for x in d[k])
        rng = lambda: np_ref.Rng(int(keys[k, 0]), int(keys[k, 1]), DEPTH)
        if k in planar_recs:
            rec, j = planar_recs[k]
        elif L is not None and 0 <= h < n_prims and int(a["mat_type"][P["mat"][h]]) in light_ref.AFFECTED:
            assert int(a["mat_type"][P["mat"][h]]) in AFFECTED_TYPES, (row["name"], "light_ref does not restate this material", h)
            rec, j = _bare_record(P, centre_of, h, ok, dk), int(P["mat"][h])
            assert rec is not None and f32(rec["t"]).view(np.uint32) == want["t"][k].view(np.uint32), (row["name"], k, h)  # (the oracle's t)
        else:
            continue
        mm = _mat_dict(rt, a, j)
        assert mm is not None, "a restated material has a constant texture"
        if k not in planar_recs:  # without a set the restatement is the oracle's own answer: the record and the material are the right ones
            al0, att0, so0, sd0, _ = np_ref.scatter(mm, dk, rec, rng())
            assert bool(al0) == bool(static["alive"][k]), (row["name"], k)
            assert not al0 or (np.array_equal(np.array(so0, f32).view(np.uint32), static["o"][k].view(np.uint32)) and
                               np.array_equal(np.array(sd0, f32).view(np.uint32), static["d"][k].view(np.uint32)) and
                               np.allclose(np.array(att0, f32), static["attenuation"][k], rtol=2e-5, atol=0)), (row["name"], k, mm)
        alive, att, so, sd, emitted, info[k] = light_ref.scatter(mm, dk, rec, rng(), L)
        restated[k] = True
        want["alive"][k] = 1 if alive else 0
        want["o"][k], want["d"][k], want["attenuation"][k] = (so, sd, att) if alive else (0, 0, 0)
        want["radiance"][k] = emitted
    return restated, info


def _statistics(rt, P, base, want, mat_type, info, stats):
    """what the coverage conditions read; -> the rays that meet a Perlin-textured primitive"""
    a, ns, n_prims = P["a"], P["ns"], P["ns"] + P["nr"]
    hit = want["hit"].astype(np.int64)
    pm = (hit >= 0) & (hit < n_prims)
    at = np.where(pm, hit, 0)
    stats["hit_fraction"] = float((hit >= 0).mean())
    stats["by_type"] = {int(t): int((mat_type == t).sum()) for t in np.unique(mat_type) if t >= 0}
    stats["sphere_hits"] = int((pm & (hit < ns) & (hit > 0)).sum())  # (the ground aside)
    stats["rect_hits"] = int((pm & (hit >= ns) & (P["chain"][at] == 0)).sum())
    stats["wrapped_hits"] = int((pm & (P["chain"][at] > 0)).sum())
    stats["deep_hits"] = int((pm & (P["chain"][at] > 4)).sum())
    stats["medium_hits"] = int(((hit >= n_prims) & (hit < base)).sum())
    perlin_ray = pm & _perlin_mats(rt, a)[P["mat"][at]]
    stats["perlin_hits"] = int(perlin_ray.sum())
    aff = [(i, t) for i, t in zip(info, mat_type) if i is not None and i["branch"] is not None]
    stats["affected"] = len(aff)
    stats["own"] = sum(1 for i, _ in aff if i["branch"] == "own")
    stats["light"] = sum(1 for i, _ in aff if i["branch"] == "light")
    stats["own_with_p_L"] = sum(1 for i, _ in aff if i["branch"] == "own" and i["p_L"] > 0)
    stats["affected_by_type"] = {t: sum(1 for _, ty in aff if ty == t) for t in AFFECTED_TYPES}
    return perlin_ray


def expected(rt, orc, row):
    """The row's scene, rays and reference, computed once: dict(B, o, d, keys, want, restated [n] bool, medium [n] bool, mat_type [n] (-1: a
    miss), static: the oracle on the scene without any set, stats: what the coverage conditions read, perlin_ray [n] bool)."""
    if row["name"] in _CACHE:
        return _CACHE[row["name"]]
    B = build(rt, row)
    scene = B["scene"]
    o, d = rays(rt, row, B)
    n = len(o)
    keys = path_keys(0, np.arange(n), np.zeros(n, np.int64))  # (the production path derives slot i's key: seed 0, pixel i, sample 0)
    P = _prims(rt, B)
    a, n_prims = P["a"], P["ns"] + P["nr"]
    base = n_prims + scene.flat.n_media  # the first planar primitive
    static = orc.debug_bounce(scene.flat_ptr, o, d, keys, depth=DEPTH, accel=orc.ACCEL_LIST)
    want = {k: v.copy() for k, v in static.items()}
    stats = {}
    centre_of = np.stack([a["sph_cx"], a["sph_cy"], a["sph_cz"]], axis=1).astype(f32)
    if B["motion"] is not None:
        _reference_motion(orc, scene, B["motion"], centre_of, o, d, keys, want, stats)
    planar_recs = _reference_quads(B["quads"], base, o, d, want, stats) if B["quads"] is not None else {}
    L = light_ref.setup(*LIGHTS) if B["lights"] is not None else None
    restated, info = _restate(rt, row, P, L, planar_recs, centre_of, o, d, keys, static, want)
    hit = want["hit"].astype(np.int64)
    medium = (hit >= n_prims) & (hit < base)
    mat_type = np.full(n, -1)
    pm = (hit >= 0) & (hit < n_prims)
    mat_type[pm] = a["mat_type"][P["mat"][hit[pm]]]
    mat_type[medium] = a["mat_type"][a["med_mat"][hit[medium] - n_prims]]
    for k, (_, j) in planar_recs.items():
        mat_type[k] = a["mat_type"][j]
    perlin_ray = _statistics(rt, P, base, want, mat_type, info, stats)
    X = dict(row=row, B=B, o=o, d=d, keys=keys, want=want, restated=restated, medium=medium, mat_type=mat_type, static=static, stats=stats, base=base,
             perlin_ray=perlin_ray)
    _CACHE[row["name"]] = X
    return X


def check_coverage(row, stats):
    """The conditions that keep a row from passing emptily, on the reference's side alone."""
    sets, form, name = row["sets"], row["form"], row["name"]
    assert stats["hit_fraction"] >= 0.5, (name, stats)
    assert stats["sphere_hits"] >= 100, (name, stats)
    if form in ("rects", "wrapped", "nested"):
        assert stats["rect_hits"] >= 100, (name, stats)
    if form in ("wrapped", "nested"):
        assert stats["wrapped_hits"] >= 100 and stats["medium_hits"] >= 100, (name, stats)
    if form == "nested":
        assert stats["deep_hits"] >= 100, (name, stats)
    if row["perlin"]:
        assert stats["perlin_hits"] >= 100, (name, stats)
    if "motion" in sets:
        assert stats["moved"] >= 100 and stats["mover_hits"] >= 100, (name, stats)
    if "quads" in sets:
        assert stats["quad_hits"] >= 100 and stats["triangle_hits"] >= 100, (name, stats)
    if "lights" in sets:
        assert all(stats["affected_by_type"][t] >= 100 for t in AFFECTED_TYPES), (name, stats)
        assert stats["own"] >= stats["affected"] // 4 and stats["light"] >= stats["affected"] // 4 and stats["own_with_p_L"] > 0, (name, stats)
    else:
        assert all(stats["by_type"].get(t, 0) >= 100 for t in ((1, 3) if row["grid"] else (1, 2, 3))), (name, stats)


# ---- the rules of the features' own tests ---------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def check_rays(got, X, what, production):
    """hit, t, alive, o and d bit for bit — except a scatter inside a medium, whose distance goes through ln(): t to 2e-6 relative and o to
    rtol 1e-5, atol 1e-4, as test_constant_medium_and_cornell_box of tests/test_gpu_parity.py holds them.  Colours of the oracle's rays as
    _check_bounce / _check_production_kernels there do (rtol 2e-5, atol 1e-6; the production kernels keep an attenuation for survivors and a
    radiance for finished paths only); of restated rays as tests/test_quads.py and _check_rays of tests/test_lights.py do: bit for bit, the
    pbr.rs materials to rtol 2e-5 with atol 0 — and the radiance of a restated finished path (an emitter of the planar set) bit for bit."""
    want, restated, medium, mat_type = X["want"], X["restated"], X["medium"], X["mat_type"]
    assert np.array_equal(got["hit"], want["hit"]), (what, "hit", int((got["hit"] != want["hit"]).sum()), np.nonzero(got["hit"] != want["hit"])[0][:5])
    assert np.array_equal(_bits(got["t"])[~medium], _bits(want["t"])[~medium]), (what, "t")
    assert np.allclose(got["t"][medium], want["t"][medium], rtol=2e-6, atol=0), (what, "t inside a medium")
    assert np.array_equal(got["alive"], want["alive"]), (what, "alive", int((got["alive"] != want["alive"]).sum()), np.nonzero(got["alive"] != want["alive"])[0][:5])
    live = want["alive"] == 1
    bad = (_bits(got["d"]) != _bits(want["d"])).any(axis=1) & live
    assert not bad.any(), (what, "d", int(bad.sum()), np.nonzero(bad)[0][:5], mat_type[bad][:5])
    bad = (_bits(got["o"]) != _bits(want["o"])).any(axis=1) & live & ~medium
    assert not bad.any(), (what, "o", int(bad.sum()), np.nonzero(bad)[0][:5], mat_type[bad][:5])
    assert np.allclose(got["o"][live & medium], want["o"][live & medium], rtol=1e-5, atol=1e-4), (what, "o inside a medium")
    exact = restated & live & ~np.isin(mat_type, PBR_TYPES)
    bad = (_bits(got["attenuation"]) != _bits(want["attenuation"])).any(axis=1) & exact
    assert not bad.any(), (what, "attenuation", int(bad.sum()), np.nonzero(bad)[0][:5], mat_type[bad][:5])
    pbr = restated & live & np.isin(mat_type, PBR_TYPES)
    assert np.allclose(got["attenuation"][pbr], want["attenuation"][pbr], rtol=2e-5, atol=0), (what, "attenuation of the pbr.rs materials")
    done = restated & ~live
    bad = (_bits(got["radiance"]) != _bits(want["radiance"])).any(axis=1) & done
    assert not bad.any(), (what, "radiance of restated finished paths", int(bad.sum()), np.nonzero(bad)[0][:5], mat_type[bad][:5])
    orc_rays = ~restated
    for key, sel in (("attenuation", orc_rays & live if production else orc_rays), ("radiance", orc_rays & ~live if production else orc_rays)):
        a, b = got[key][sel].astype(np.float64), want[key][sel].astype(np.float64)
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin), (what, key)
        assert np.allclose(a[fin], b[fin], rtol=2e-5, atol=1e-6), (what, key, np.abs(a[fin] - b[fin]).max())
    if production:
        assert not got["radiance"][live].any(), what  # emitted = 0 for everything that scatters (material.rs:12-14)
