"""The frames of tests/test_frame_replay.py: the smallest geometries at which the frame arithmetic takes another path, the sets they are
rendered under, the two scenes, and a numpy restatement of that arithmetic (rt_frame_plan.h, rt_kernels.h) which
tests/test_frame_cases_host.py uses to show that every geometry has the property it is named for."""
import numpy as np

import light_ref
from helpers import ctr_draw

f32 = np.float32
SEED, SPP, MAX_DEPTH = 77, 5, 7
SPP_ADAPTIVE = 6  # the maximum of the adaptive cases: their replays hold six samples, the frames use the first five

# ---- geometries -----------------------------------------------------------------------------------------------------------------------
# name: nx, ny, (band, count) of a sharded one, `shard`: the shard the geometry is named for
GEOMETRIES = {
    "1x1": dict(nx=1, ny=1),                                        # a single pixel
    "7x3": dict(nx=7, ny=3),                                        # row-major, under a chunk
    "32x5": dict(nx=32, ny=5),                                      # nx % 8 == 0 but fewer than 8 rows: no tiles
    "16x11": dict(nx=16, ny=11),                                    # tiles plus a 3-row tail, under a chunk
    "24x13": dict(nx=24, ny=13),                                    # tiles plus a tail, 312 pixels: a chunk straddles samples
    "24x27/8x2": dict(nx=24, ny=27, band=8, count=2, shard=1),      # shard 1 owns 11 rows: tiles plus a tail inside a shard
    "16x11/4x4": dict(nx=16, ny=11, band=4, count=4, shard=2),      # shard 2 has a partial band, shard 3 has no row
}
TAILED = ("16x11", "24x13", "24x27/8x2")  # tiles plus a tail
EVERY_SET_GETS = ("7x3",) + TAILED

# ---- sets -----------------------------------------------------------------------------------------------------------------------------
LENS_SPHERES, LENS_GENERAL = (0.04, 7.5), (0.1, 9.0)
SHUTTER = (0.2, 0.9)
SETS = {  # name: scene, then what is set
    "none": dict(scene="spheres"),
    "lens": dict(scene="spheres", lens=LENS_SPHERES),
    "motion": dict(scene="spheres", motion=True),
    "motion+lens": dict(scene="spheres", motion=True, lens=LENS_SPHERES),
    "s-lights": dict(scene="spheres", lights=True),
    "quads": dict(scene="general", quads=True),
    "g-lights": dict(scene="general", lights=True),
    "quads+lights": dict(scene="general", quads=True, lights=True),
    "quads+lights+lens": dict(scene="general", quads=True, lights=True, lens=LENS_GENERAL),
}
EVERY_GEOMETRY_GETS = ("none", "lens", "quads")
CASES = [(s, g) for s in SETS for g in GEOMETRIES if s in EVERY_GEOMETRY_GETS or g in EVERY_SET_GETS]
ADAPTIVE_CASES = [(s, g) for s in ("lens", "motion") for g in TAILED]
MULTI_CASES = [(s, "24x13") for s in SETS]  # one case per set through MultiRenderer
DENOISE_CASE = ("lens", "24x13")


def case_id(case):
    return "%s-%s" % case


def params(rt, geom, spp=SPP, shard_id=None, **kw):
    """RtParams of a geometry: the whole frame, or shard `shard_id` of a sharded one"""
    g = GEOMETRIES[geom]
    if shard_id is not None:
        kw = dict(kw, shard_band=g["band"], shard_count=g["count"], shard_id=shard_id)
    return rt.make_params(g["nx"], g["ny"], spp, **{"max_depth": MAX_DEPTH, "seed": SEED, **kw})


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
N_SMALL = 36
SPHERES_MATS = ("diffuse", "diffuse", "metal", "dielectric", "diffuse", "emission")


def vfov(aspect):
    """40 degrees, less for a wide frame: its columns stay over the middle of the scene"""
    return min(40.0, 60.0 / aspect)


def sphere_scene(rt, aspect):
    """Sphere-only, near the origin, under the gradient sky: a ground (radius 100), a ball of radius 12 hanging over the middle that sends
    about half of what leaves the ground back down — so that paths live for several bounces, a few reach the depth limit, and most end in
    light — and one jittered 6 x 6 layer of 36 small spheres clear of the ground: Diffuse, Metal, Dielectric and Emission.  Every small
    sphere but the emitters moves under the motion set.  (A ground of radius 1000 rendered the same frames as its replay, but the two
    single-kernel hooks then parted on a few rays: with a light set a path now and then gets inside the ground, its next ray is 1000 to
    2000 units long, and at that distance Sphere::hit in f32 reports small spheres near the exit that the tree rightly culls.)
    Returns (scene, movers, their centres at time 1, light parallelograms)."""
    f = rt._ffi
    rng = np.random.default_rng(5)
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    mats = {"diffuse": s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.75, 0.6, 0.5))), "metal": s.material(f.MAT_METAL, color=(0.8, 0.8, 0.7), p=(0.9,)),
            "dielectric": s.material(f.MAT_DIELECTRIC, p=(1.5,)), "emission": s.material(f.MAT_EMISSION, tex0=s.constant_tex((4.0, 3.5, 3.0))),
            "white": s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.8, 0.8, 0.8)))}
    s.sphere((0.0, -100.0, 0.0), 100.0, mats["white"], "ground")
    s.sphere((0.0, 16.0, 0.0), 12.0, mats["white"], "ball")
    ix, iz = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    c0 = np.stack([-3.25 + 1.3 * ix.ravel() + rng.uniform(-0.15, 0.15, N_SMALL), rng.uniform(0.5, 2.4, N_SMALL),
                   -3.25 + 1.3 * iz.ravel() + rng.uniform(-0.15, 0.15, N_SMALL)], axis=1).astype(f32)
    kinds = [SPHERES_MATS[int(k)] for k in rng.permutation(N_SMALL) % len(SPHERES_MATS)]
    for k in range(N_SMALL):
        s.sphere(tuple(float(x) for x in c0[k]), 0.3, mats[kinds[k]], "s%d" % k)
    s.set_camera((5.5, 3.6, 4.5), (0.0, 0.6, 0.0), (0, 1, 0), vfov(aspect), aspect)
    scene = s.finish()
    movers = np.array([2 + k for k in range(N_SMALL) if kinds[k] != "emission"], dtype=np.uint32)
    c1 = (c0[movers - 2] + rng.uniform(-0.2, 0.2, (len(movers), 3))).astype(f32)
    c1[:, 1] = np.clip(c1[:, 1], 0.5, 3.0)
    lights = ([[-1.5, 3.2, -1.5], [1.0, 0.4, 2.0]], [[3.0, 0.0, 0.0], [0.0, 1.2, 0.0]], [[0.0, 0.0, 3.0], [1.2, 0.0, -0.6]])
    return scene, movers, c1, lights


def general_scene(rt, aspect):
    """A small general scene after test_quads._general_scene, with emitters: the ground and the ball of sphere_scene, 14 spheres, a rotated
    and translated box, a constant medium, an emitting rectangle and a diffuse one; as planar primitives 60 triangles, a metal quad, an
    emitting quad and a patch over the ground.  Scene.lights finds the two emitters."""
    f = rt._ffi
    rng = np.random.default_rng(23)
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    mats = [s.material(f.MAT_DIFFUSE, tex0=s.constant_tex(tuple(float(x) for x in rng.uniform(0.3, 0.9, 3)))) for _ in range(2)]
    mats.append(s.material(f.MAT_LAMBERT, tex0=s.constant_tex((0.5, 0.7, 0.6))))
    mats.append(s.material(f.MAT_METAL, color=(0.8, 0.7, 0.6), p=(0.9,)))
    mats.append(s.material(f.MAT_DIELECTRIC, p=(1.5,)))
    light = s.material(f.MAT_EMISSION, tex0=s.constant_tex((6.0, 5.5, 5.0)))
    s.sphere((0.0, -100.0, 0.0), 100.0, mats[0], "ground")
    s.sphere((0.0, 16.5, 0.0), 12.0, mats[1], "ball")
    for k in range(14):
        s.sphere((float(rng.uniform(-3.5, 3.5)), 0.35, float(rng.uniform(-3.5, 3.5))), 0.35, mats[k % 5], "s%d" % k)
    s.translate(s.rotate_y(s.gbox((0.0, 0.0, 0.0), (1.0, 1.4, 1.0), mats[0]), 20.0), (1.8, 0.0, -1.0))
    s.constant_medium(s.gbox((-3.0, 0.0, 0.5), (-1.6, 1.2, 1.9), mats[0]), 0.8, s.constant_tex((0.9, 0.9, 0.9)))
    s.rect(f.RECT_XZ, (-1.2, 3.6, -1.2), (1.2, 3.6, 1.2), light)
    s.rect(f.RECT_XY, (-3.5, 0.0, -3.8), (3.5, 2.5, -3.8), mats[2])
    for k in range(60):
        a = rng.uniform(-3.2, 3.2, 3) * [1, 0, 1] + [0, rng.uniform(0.3, 2.6), 0]
        s.triangle(tuple(a), tuple(a + rng.normal(size=3) * 0.8), tuple(a + rng.normal(size=3) * 0.8), mats[k % 5])
    s.quad((-1.5, 2.8, -2.5), (3.0, 0.0, 0.5), (0.0, 0.5, 2.0), mats[3])
    s.quad((2.6, 0.6, -0.8), (0.0, 1.0, 0.0), (0.6, 0.0, 1.4), light)
    s.quad((0.5, 0.03, 0.5), (3.0, 0.0, 0.0), (0.0, 0.0, 3.0), mats[2])  # a patch just over the ground, in front of the camera
    s.set_camera((7.0, 4.2, 5.5), (0.0, 0.5, 0.0), (0, 1, 0), vfov(aspect), aspect)
    return s.finish()


def material_type_of_hit(scene, quads_on):
    """hit index of debug_bounce -> the material type shade() reads: spheres, rectangles, media (their phase function), then the planar
    primitives when the set is on; -1 for a miss is left to the caller."""
    a = scene.arrays()
    mat = np.concatenate([a["sph_mat"], a["rect_mat"], a["med_mat"]]).astype(np.int64)
    if quads_on:
        q = scene.quads
        mat = np.concatenate([mat, np.ctypeslib.as_array(q.mat, shape=(q.n,)).astype(np.int64)])
    return a["mat_type"].astype(np.int64)[mat]


def takes_light_branch(keys, depth, mat_type):
    """light_ref.scatter on a hit of an affected material: the first draw of the depth (counter (depth + 1) * 256, np_ref.Rng) selects the
    light when it is >= 0.5"""
    s = ((ctr_draw(keys[:, 0].astype(np.uint64), keys[:, 1].astype(np.uint64), (depth + 1) * 256) >> 8).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)
    return np.isin(mat_type, light_ref.AFFECTED) & (s >= f32(0.5))


# ---- the frame arithmetic, restated (rt_frame_plan.h, rt_kernels.h) ----------------------------------------------------------------
def shard_rows(ny, band, count, sid):
    """rt_shard_rows by counting: the rows j with (j // band) % count == sid"""
    if count <= 1:
        return ny
    band = band or 1
    if sid >= count:
        return 0
    return sum(1 for j in range(ny) if (j // band) % count == sid)


def pixel_order(po, general, nx, rows):
    """(tiles_per_row, tile_pixels): 8 x 8 tiles when nx % 8 == 0, rows >= 8 and the scene (or RT_OPT_PIXEL_ORDER 2) wants them"""
    want = (po == 2) if po else not general
    tpr = nx // 8 if (nx % 8 == 0 and rows >= 8 and want) else 0
    return tpr, tpr * 64 * (rows // 8)


def local_of_pixel(nx, tpr, tile_pixels, i, lj):
    """where the path slots keep pixel (i, local row lj): tiles first, the last rows % 8 rows row-major behind them"""
    if tpr == 0 or lj * nx >= tile_pixels:
        return lj * nx + i
    return ((lj >> 3) * tpr + (i >> 3)) * 64 + (lj & 7) * 8 + (i & 7)


def shard_cap(nq, n_max):
    return -(-(-(-n_max // 256)) // nq) * 256


def deal(nq, idx):
    """path idx of a slice -> (queue shard, position): chunks of 256 consecutive paths go round the shards"""
    chunk = idx // 256
    return chunk % nq, (chunk // nq) * 256 + idx % 256


def properties(geom, general=False, po=0):
    """What a geometry reaches, per shard with rows (and "empty": the shards without)."""
    g = GEOMETRIES[geom]
    band, count = g.get("band", 0), g.get("count", 1)
    out = {"empty": [k for k in range(count) if shard_rows(g["ny"], band, count, k) == 0], "shards": {}}
    for k in range(count):
        rows = shard_rows(g["ny"], band, count, k)
        if rows == 0:
            continue
        npix = rows * g["nx"]
        tpr, tp = pixel_order(po, general, g["nx"], rows)
        last_band = rows % (band or 1) if count > 1 else 0
        straddles = any((c * 256) // npix != (min(c * 256 + 255, npix * SPP - 1)) // npix for c in range(-(-npix * SPP // 256)))
        out["shards"][k] = dict(rows=rows, npix=npix, tiles_per_row=tpr, tile_pixels=tp, tail_rows=rows % 8 if tpr else 0,
                                partial_band=last_band, chunk_straddles_samples=straddles)
    return out
