"""Planar primitives on the GPU (rt_set_quads).  Static frames do not move by one bit; single rays equal the numpy restatement
(tests/quad_ref.py) in hit and t, bit for bit, under every flag; an axis-aligned quad is the reference's rectangle; whole images of
black quads and triangles equal the restatement exactly; every search path agrees outright; invalid sets are refused.

The scattered ray and attenuation of every hit of the single-ray test come from tests/golden/np_ref.py's scatter on the record
tests/quad_ref.py builds."""
import numpy as np
import pytest

import lens_ref
import quad_ref

pytestmark = pytest.mark.gpu
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, what=""):
    assert np.array_equal(_bits(a[0]), _bits(b[0])), what
    assert a[2].n_rays == b[2].n_rays and list(a[2].rays_per_depth) == list(b[2].rays_per_depth), what


@pytest.fixture
def fresh(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


def _some_quads(rt, scale=1.0, at=(0.0, 1.0, 0.0)):
    c = np.array(at, f32)
    q = np.array([c + f32([-1, 0, 0]) * scale, c + f32([0.2, 0.1, 0.5]) * scale], f32)
    u = np.array([[1.5, 0.3, 0.2], [0.0, 1.0, 0.4]], f32) * f32(scale)
    v = np.array([[0.1, 1.2, -0.3], [0.9, 0.1, -0.5]], f32) * f32(scale)
    return rt.make_quads(q, u, v, [0, 1], [0, 0])


# ---- 1. static frames do not move -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nx,ny,spp,depth,scale,at", [("sphere_scene", 160, 90, 8, 12, 1.0, (0, 1, 0)), ("cornell_box", 96, 96, 8, 12, 150.0, (278, 200, 278)),
                                                            ("final_scene", 96, 96, 6, 8, 120.0, (278, 278, 200))])
def test_static_frames_do_not_move(rt, fresh, name, nx, ny, spp, depth, scale, at):
    scene = rt.Scene.build(name, nx / ny)
    p = rt.make_params(nx, ny, spp, max_depth=depth, seed=7)
    fresh.upload(scene)
    info0 = fresh.scene_info()
    never = fresh.render(scene.camera, p)
    fresh.set_quads(None)
    _same(never, fresh.render(scene.camera, p), "set to NULL")
    quads = _some_quads(rt, scale, at)
    fresh.set_quads(quads)
    assert fresh.scene_info()["n_planar"] == 2 and fresh.scene_info() != info0
    with_set = fresh.render(scene.camera, p)
    assert not np.array_equal(_bits(with_set[0]), _bits(never[0])), "the set must be visible"
    fresh.set_quads(rt.make_quads(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), [], []))
    assert fresh.scene_info() == info0
    _same(never, fresh.render(scene.camera, p), "set, then cleared with n == 0")
    fresh.set_quads(quads)
    fresh.upload(scene)  # an upload clears the set
    assert fresh.scene_info() == info0
    _same(never, fresh.render(scene.camera, p), "an upload clears the set")


# ---- 2. single rays ---------------------------------------------------------------------------------------------------------------
MIXED_MATS = [{"type": 1, "tex": (0.7, 0.3, 0.2)}, {"type": 3, "color": (0.8, 0.7, 0.6), "p0": 0.1}, {"type": 4, "p0": 1.5}, {"type": 1, "image": True}]
MIXED_SPHERES = [((-1.5, 0.5, 1.0), 0.7, 0), ((1.8, -0.6, 0.4), 0.6, 1), ((0.2, 1.6, -1.0), 0.8, 2), ((-0.5, -1.8, 2.0), 0.5, 1)]
MIXED_RECT = ((-3.0, -1.0, -3.0), (3.0, -1.0, 3.0), 0)  # XZ, y = -1: it cuts through the figures


def _mixed_scene(rt):
    """spheres and a rectangle AMONG the quads and triangles (rays hit all of them), Diffuse, Metal, Dielectric and an image-textured Diffuse"""
    f = rt._ffi
    rng = np.random.default_rng(5)
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    mats = [s.material(f.MAT_DIFFUSE, tex0=s.constant_tex(MIXED_MATS[0]["tex"])), s.material(f.MAT_METAL, color=MIXED_MATS[1]["color"], p=(0.1,)),
            s.material(f.MAT_DIELECTRIC, p=(1.5,)), s.material(f.MAT_DIFFUSE, tex0=s.image_tex("res/earthmap.jpg"))]
    for k, (c, r, m) in enumerate(MIXED_SPHERES):
        s.sphere(c, r, mats[m], "s%d" % k)
    s.rect(f.RECT_XZ, MIXED_RECT[0], MIXED_RECT[1], mats[MIXED_RECT[2]])
    for k in range(12):
        q = rng.uniform(-3, 3, 3)
        u, v = rng.normal(size=3) * 1.5, rng.normal(size=3) * 1.5
        if k % 2:
            s.triangle(tuple(q), tuple(q + u), tuple(q + v), mats[k % 4])
        else:
            s.quad(tuple(q), tuple(u), tuple(v), mats[k % 4])
    s.set_camera((0, 0, 12), (0, 0, 0), (0, 1, 0), 40.0, 1.0)
    return s.finish(use_bvh=False)


def _quad_arrays(quads):
    n = quads.n
    g = lambda p, k, t: np.ctypeslib.as_array(p, shape=(n * k,)).reshape((n, k) if k > 1 else (n,)).astype(t)
    return g(quads.q, 3, f32), g(quads.u, 3, f32), g(quads.v, 3, f32), g(quads.kind, 1, np.uint8), g(quads.mat, 1, np.uint32)


def _class_rays(q, u, v, kind, rng, m):
    """rays by class: 0 random, 1 grazing an edge, 2 aimed at a corner, 3 from behind, 4 nearly parallel to the plane, 5 at the spheres
    and the rectangle"""
    n = len(q)
    cls = rng.integers(0, 6, m)
    i = rng.integers(0, n, m)
    a, b = rng.uniform(0.05, 0.45, m), rng.uniform(0.05, 0.45, m)
    a[cls == 1] = rng.choice([0.0, 1e-7, -1e-7], (cls == 1).sum())
    a[cls == 2], b[cls == 2] = 0.0, 0.0
    q64, u64, v64 = q.astype(np.float64), u.astype(np.float64), v.astype(np.float64)
    tgt = q64[i] + a[:, None] * u64[i] + b[:, None] * v64[i]
    nh = np.cross(u64[i], v64[i])
    nh /= np.linalg.norm(nh, axis=1)[:, None]
    org = tgt + nh * rng.uniform(2, 6, (m, 1)) + rng.normal(size=(m, 3))
    org[cls == 3] = (tgt - nh * rng.uniform(2, 6, (m, 1)) + rng.normal(size=(m, 3)))[cls == 3]
    par = cls == 4
    side = u64[i] / np.linalg.norm(u64[i], axis=1)[:, None]
    org[par] = (tgt + side * 3.0 + nh * 10.0 ** rng.uniform(-9, -6, (m, 1)))[par]
    oth = cls == 5
    cen = np.array([c for c, _, _ in MIXED_SPHERES] + [(0.0, -1.0, 0.0)])
    tgt[oth] = (cen[rng.integers(0, len(cen), m)] + rng.normal(size=(m, 3)) * [0.4, 0.4, 0.4])[oth]
    org[oth] = (rng.normal(size=(m, 3)) * 4 + [0, 3, 0])[oth]
    d = tgt - org
    d /= np.linalg.norm(d, axis=1)[:, None]
    return org.astype(f32), d.astype(f32), cls


_MIXED = {}


def _mixed_expected(rt):
    """the scene, the rays and what tests/quad_ref.py + tests/golden/np_ref.py make of them (computed once for the four flag sets)"""
    if _MIXED:
        return _MIXED
    from helpers import path_keys
    import os
    import ray_tracing_in_one_weekend_amd.images as images
    scene = _mixed_scene(rt)
    image = rt.decode_rgb32f(os.path.join(images.ASSET_DIR, "res/earthmap.jpg"))
    q, u, v, kind, mat = _quad_arrays(scene.quads)
    rng = np.random.default_rng(11)
    m = 6144
    o, d, cls = _class_rays(q, u, v, kind, rng, m)
    keys = path_keys(0, np.arange(m), np.zeros(m, np.int64))  # (the production path derives slot i's key: seed 0, pixel i, sample 0)
    depth = 1
    ns = len(MIXED_SPHERES)
    base = ns + 1
    assert base == scene.flat.n_spheres + scene.flat.n_rects + scene.flat.n_media
    # the entries in front of the set: HitableList::hit over spheres, then the rectangle (t_max shrinks, a later equal root wins)
    t0, hit0, rec0 = np.full(m, np.finfo(f32).max, f32), np.full(m, -1, np.int64), [None] * m
    for k in range(m):
        ok, dk = tuple(f32(x) for x in o[k]), tuple(f32(x) for x in d[k])
        t_max = f32(np.finfo(f32).max)
        for s_, (c, r, _) in enumerate(MIXED_SPHERES):
            h = np_ref_mod().sphere_hit(np_ref_mod().v3(*c), f32(r), ok, dk, f32(1e-3), t_max)
            if h is not None:
                hit0[k], t_max, rec0[k] = s_, f32(h["t"]), h
        h = np_ref_mod().rect_hit(1, np_ref_mod().v3(*MIXED_RECT[0]), np_ref_mod().v3(*MIXED_RECT[1]), ok, dk, f32(1e-3), t_max)
        if h is not None and not np.isnan(h["t"]):
            hit0[k], t_max, rec0[k] = ns, f32(h["t"]), h
        t0[k] = t_max
    alone = quad_ref.closest(q, u, v, kind, o, d, base=base)
    hit, t, al, be = quad_ref.closest(q, u, v, kind, o, d, base=base, t0=t0, hit0=hit0)
    normal, _, _ = quad_ref.setup(q, u, v)
    # the flattened material order is the scene's business: planar primitive i names flat material mat[i], and which of MIXED_MATS
    # that is is read from the flat tables (type, and for the two Diffuse ones the texture: constant colour or image)
    arrs = scene.arrays()

    def mixed_of_flat(j):
        ty = int(arrs["mat_type"][j])
        if ty != 1:
            return {3: 1, 4: 2}[ty]
        tex = int(arrs["mat_tex0"][j])
        if int(arrs["tex_type"][tex]) == rt._ffi.TEX_IMAGE:
            return 3
        assert int(arrs["tex_type"][tex]) == rt._ffi.TEX_CONSTANT
        assert np.array_equal(arrs["tex_color0"][3 * tex:3 * tex + 3], np.array(MIXED_MATS[0]["tex"], f32))
        return 0
    mat_of = np.array([mixed_of_flat(int(mat[i])) for i in range(len(q))])
    assert np.array_equal(mat_of, np.arange(len(q)) % 4)  # _mixed_scene gave figure k the material k % 4
    want = {"hit": hit.astype(np.int32), "t": np.where(hit >= 0, t, f32(0)).astype(f32), "alive": np.zeros(m, np.uint8),
            "o": np.zeros((m, 3), f32), "d": np.zeros((m, 3), f32), "attenuation": np.zeros((m, 3), f32)}
    for k in range(m):
        if hit[k] < 0:
            continue
        if hit[k] >= base:
            i = int(hit[k]) - base
            rec = quad_ref.hit_record(normal[i], o[k], d[k], t[k], al[k], be[k])
            mm = MIXED_MATS[mat_of[i]]
        else:
            rec = rec0[k]
            mm = MIXED_MATS[MIXED_SPHERES[hit[k]][2] if hit[k] < ns else MIXED_RECT[2]]
        alive, att, so, sd, _ = quad_ref.scatter(mm, image, rec, d[k], keys[k], depth)
        if alive:
            want["alive"][k], want["o"][k], want["d"][k], want["attenuation"][k] = 1, so, sd, att
    _MIXED.update(scene=scene, o=o, d=d, keys=keys, cls=cls, want=want, base=base, ns=ns, alone=alone, t0=t0, hit0=hit0, depth=depth,
                  q=q, u=u, v=v, mat_of=mat_of)
    return _MIXED


def np_ref_mod():
    return quad_ref.np_ref


@pytest.mark.parametrize("flags", ["0", "brute", "production", "both"])
def test_single_rays_equal_the_restatement(rt, fresh, flags):
    f = rt._ffi
    fl = {"0": 0, "brute": f.FLAG_BRUTE_FORCE, "production": f.FLAG_PRODUCTION_KERNELS, "both": f.FLAG_BRUTE_FORCE | f.FLAG_PRODUCTION_KERNELS}[flags]
    X = _mixed_expected(rt)
    scene, o, d, cls, want, base, ns = X["scene"], X["o"], X["d"], X["cls"], X["want"], X["base"], X["ns"]
    m = len(o)
    fresh.upload(scene)
    fresh.set_quads(scene.quads)
    got = fresh.debug_bounce(o, d, X["keys"], depth=X["depth"], flags=fl)
    hit = want["hit"]
    assert np.array_equal(got["hit"], hit), int((got["hit"] != hit).sum())
    assert np.array_equal(_bits(got["t"]), _bits(want["t"]))
    assert np.array_equal(got["alive"], want["alive"]), int((got["alive"] != want["alive"]).sum())
    for key in ("o", "d", "attenuation"):
        bad = (_bits(got[key]) != _bits(want[key])).any(axis=1) & (want["alive"] == 1)
        assert not bad.any(), (key, int(bad.sum()), np.nonzero(bad)[0][:5], hit[bad][:5])
    # each class of ray is represented, hits and misses; the 1e-8 branch is taken
    for c in range(6):
        assert (cls == c).sum() > m // 10
    planar = hit >= base
    assert 0.3 < planar[cls == 0].mean() and 0.05 < planar[cls == 1].mean() < 0.999 and planar[cls == 3].mean() > 0.3
    normal, _, _ = quad_ref.setup(X["q"], X["u"], X["v"])
    den = np.abs(np.einsum("mk,nk->mn", d.astype(np.float64), normal.astype(np.float64)))
    assert (den[cls == 4].min(axis=1) < 1e-8).sum() > 20
    # the winner rule between the set and what precedes it: spheres and the rectangle are hit, and where a ray has a candidate of
    # both kinds each kind wins some
    assert ((hit >= 0) & (hit < ns)).sum() > 200 and (hit == ns).sum() > 200
    both = (X["hit0"] >= 0) & (X["alone"][0] >= 0)
    assert (both & planar).sum() > 100 and (both & ~planar).sum() > 100
    # every material of the set scatters checked rays, the image-textured one among them
    for mm in range(4):
        sel = planar & (want["alive"] == 1)
        sel[planar] &= X["mat_of"][hit[planar] - base] == mm
        assert sel.sum() > 50, mm
    img_att = want["attenuation"][planar & (want["alive"] == 1)]
    assert len(np.unique(img_att, axis=0)) > 50  # many different texels were read through (alpha, beta)


# ---- 3. tie to the reference's rectangles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("winding", [0, 1])
def test_axis_aligned_quad_is_the_rectangle(rt, fresh, axis, winding):
    f = rt._ffi
    rect_axis = {0: f.RECT_YZ, 1: f.RECT_XZ, 2: f.RECT_XY}[axis]
    ua, va = [(1, 2), (0, 2), (0, 1)][axis]
    mn, mx = np.array([-1.25, 0.5, -0.75], f32), np.array([2.0, 3.25, 1.5], f32)
    mx[axis] = mn[axis]
    ext = (mx - mn).astype(f32)
    U, V = np.zeros(3, f32), np.zeros(3, f32)
    U[ua], V[va] = ext[ua], ext[va]
    if winding:
        U, V = V, U

    def make(as_quad):
        s = rt.Scene.new()
        s.set_sky(f.SKY_GRADIENT)
        m = s.material(f.MAT_METAL, color=(0.8, 0.7, 0.6), p=(0.2,))
        s.sphere((400, 400, 400), 0.5, m, "away")
        if as_quad:
            s.quad(tuple(mn), tuple(U), tuple(V), m)
        else:
            s.rect(rect_axis, tuple(mn), tuple(mx), m)
        s.set_camera((0, 0, 12), (0, 0, 0), (0, 1, 0), 40.0, 1.0)
        return s.finish(use_bvh=False)
    rng = np.random.default_rng(100 + 2 * axis + winding)
    m = 8192
    tgt = mn + rng.uniform(-0.15, 1.15, (m, 3)) * ext
    org = tgt + rng.normal(size=(m, 3)) * 3 + np.eye(3)[axis] * rng.choice([-5.0, 5.0], (m, 1))
    d = tgt - org
    d /= np.linalg.norm(d, axis=1)[:, None]
    o, d = org.astype(f32), d.astype(f32)
    keys = rng.integers(0, 2 ** 32, (m, 2), dtype=np.uint64).astype(np.uint32)
    a, b = make(False), make(True)
    fresh.upload(a)
    ra = fresh.debug_bounce(o, d, keys, depth=1)
    fresh.upload(b)
    fresh.set_quads(b.quads)
    rb = fresh.debug_bounce(o, d, keys, depth=1)
    # a ray whose float64 hit point lies within 1e-5 of the extent from an edge may fall on either side of alpha, beta = 0, 1
    t64 = (float(mn[axis]) - o[:, axis].astype(np.float64)) / d[:, axis].astype(np.float64)
    P = o.astype(np.float64) + d.astype(np.float64) * t64[:, None]
    near = np.zeros(m, bool)
    for k in (ua, va):
        e = 1e-5 * float(ext[k])
        near |= (np.abs(P[:, k] - float(mn[k])) < e) | (np.abs(P[:, k] - float(mx[k])) < e)
    assert near.mean() <= 1e-3
    keep = ~near
    ha, hb = ra["hit"] >= 0, rb["hit"] >= 0
    assert np.array_equal(ha[keep], hb[keep]) and 0.3 < ha.mean() < 0.9
    # (the world normal of a quad wound the other way is -axis; set_face_normal turns both towards the ray: the same record)
    for key in ("t", "o", "d", "attenuation", "alive"):
        assert np.array_equal(_bits(ra[key][keep]) if ra[key].dtype != np.uint8 else ra[key][keep], _bits(rb[key][keep]) if rb[key].dtype != np.uint8 else rb[key][keep]), key


# ---- 4. exact image -----------------------------------------------------------------------------------------------------------------
def _black_scene(rt):
    f = rt._ffi
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    black = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.0, 0.0, 0.0)))
    s.quad((-3, -1, -1), (2.5, 0.4, 0.3), (0.2, 2.0, -0.6), black)
    s.triangle((0.5, -1.5, 0.5), (3.0, -0.5, -1.0), (1.0, 2.0, 0.0), black)
    s.triangle((-1.0, 1.0, 1.0), (0.5, 1.2, 1.5), (-0.4, 2.4, 0.8), black)
    s.set_camera((0, 0, 9), (0, 0, 0), (0, 1, 0), 40.0, 1.0)
    return s.finish(use_bvh=False)


@pytest.mark.parametrize("lens", [None, (0.3, 9.0)])
@pytest.mark.parametrize("spp", [1, 4])
def test_exact_image_of_black_quads_and_triangles(rt, fresh, lens, spp):
    scene = _black_scene(rt)
    nx = ny = 64
    p = rt.make_params(nx, ny, spp, max_depth=0, seed=3)
    fresh.upload(scene)
    fresh.set_quads(scene.quads)
    if lens:
        fresh.set_lens(lens)
    img = fresh.render(scene.camera, p)[0]
    q, u, v, kind, _ = _quad_arrays(scene.quads)
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    acc = np.zeros((ny * nx, 3), f32)
    covered = np.zeros(ny * nx, bool)
    for s_ in range(spp):
        o, d, _ = lens_ref.lens_rays(scene.camera, p, ii.ravel(), jj.ravel(), np.full(nx * ny, s_), lens[0] if lens else 0.0, lens[1] if lens else 1.0)
        hit, _, _, _ = quad_ref.closest(q, u, v, kind, o, d)
        col = lens_ref.sky_gradient(d)
        col[hit >= 0] = 0.0
        covered |= hit >= 0
        acc = (acc + col).astype(f32)  # the in-order f32 sum of k_resolve
    ref = (acc / f32(spp)).astype(f32).reshape(ny, nx, 3)
    assert 0.05 < covered.mean() < 0.6  # the figures are in view
    assert np.array_equal(_bits(img), _bits(ref))


# ---- 5. every search path agrees, outright ----------------------------------------------------------------------------------------------
def _general_scene(rt, n_tri=240):
    f = rt._ffi
    rng = np.random.default_rng(17)
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    mats = [s.material(f.MAT_DIFFUSE, tex0=s.constant_tex(tuple(float(x) for x in rng.uniform(0.2, 0.9, 3)))) for _ in range(3)]
    mats.append(s.material(f.MAT_METAL, color=(0.8, 0.7, 0.6), p=(0.05,)))
    mats.append(s.material(f.MAT_DIELECTRIC, p=(1.5,)))
    s.sphere((0.0, -1000.0, 0.0), 1000.0, mats[1], "ground")
    for k in range(30):
        s.sphere((float(rng.uniform(-6, 6)), 0.3, float(rng.uniform(-6, 6))), 0.3, mats[k % 5], "s%d" % k)
    s.translate(s.rotate_y(s.gbox((0.0, 0.0, 0.0), (1.0, 1.4, 1.0), mats[0]), 20.0), (2.5, 0.0, -1.0))
    s.constant_medium(s.gbox((-3.5, 0.0, 0.5), (-2.0, 1.2, 2.0), mats[0]), 0.8, s.constant_tex((0.9, 0.9, 0.9)))
    for k in range(n_tri):
        a = rng.uniform(-5, 5, 3) * [1, 0, 1] + [0, rng.uniform(0.2, 2.5), 0]
        s.triangle(tuple(a), tuple(a + rng.normal(size=3) * 0.6), tuple(a + rng.normal(size=3) * 0.6), mats[k % 5])
    s.quad((-1.5, 3.0, -1.5), (3.0, 0.0, 0.5), (0.0, 0.4, 3.0), mats[3])
    s.set_camera((13, 4, 5), (0, 0.4, 0), (0, 1, 0), 25.0, 16 / 9)
    return s.finish()


@pytest.mark.parametrize("which", ["quads_scene", "mesh_scene", "general"])
def test_every_search_path_agrees(rt, fresh, which):
    f = rt._ffi
    nx, ny, spp, depth = (96, 96, 6, 8) if which != "general" else (128, 72, 6, 8)
    scene = _general_scene(rt) if which == "general" else rt.Scene.build(which, nx / ny)
    p = rt.make_params(nx, ny, spp, max_depth=depth, seed=21)

    def render(opts=(), flags=0, **kw):
        for k, val in opts:
            fresh.set_option(k, val)
        fresh.upload(scene)
        fresh.set_quads(scene.quads)
        out = fresh.render(scene.camera, rt.make_params(nx, ny, spp, max_depth=depth, seed=21, flags=flags, **kw))
        info = fresh.scene_info()
        for k, _ in opts:
            fresh.set_option(k, 0)
        return out, info
    base, info = render()
    if which != "mesh_scene":  # (5 122 leaves do not fit the 80 KB of two workgroups per CU: mesh_scene's tree goes through L2 by itself)
        assert info["tree_in_lds"] == 1
    else:
        assert info["tree_in_lds"] == 0
    if which == "general":
        assert info["general_tables_in_lds"] == 1
    assert info["n_planar"] == scene.quads.n and info["general_kernels"] == 1 and info["grid"] == 0 and info["plane_data_in_lds"] == 0
    hbm, info_hbm = render([("tree_placement", 1)])
    assert info_hbm["tree_in_lds"] == 0
    _same(base, hbm, "tree through L2")
    no_glds, info_no_glds = render([("general_lds", 1)])
    assert info_no_glds["general_tables_in_lds"] == 0
    _same(base, no_glds, "tables not in LDS")
    _same(base, render(flags=f.FLAG_BRUTE_FORCE)[0], "list walk")
    _same(base, render(spp_slice=2)[0], "3 slices")
    # 4 shards, de-interleaved
    full = np.zeros_like(base[0])
    for sid in range(4):
        fresh.upload(scene)
        fresh.set_quads(scene.quads)
        ps = rt.make_params(nx, ny, spp, max_depth=depth, seed=21, shard_band=8, shard_count=4, shard_id=sid)
        part = fresh.render(scene.camera, ps)[0]
        rows = [fresh._lib.rt_shard_row_to_image_row(r, 8, 4, sid) for r in range(part.shape[0])]
        full[rows] = part
    assert np.array_equal(_bits(full), _bits(base[0])), "4 shards"
    m = rt.MultiRenderer([0, 0], copy_gather=True)
    try:
        m.upload(scene)
        m.set_quads(scene.quads)
        assert np.array_equal(_bits(m.render(scene.camera, p)[0]), _bits(base[0])), "two contexts, copy gather"
    finally:
        m.close()


def test_20480_triangles_tree_against_list_walk(rt, fresh):
    f = rt._ffi
    rng = np.random.default_rng(9)
    n = 20480
    a = rng.uniform(-10, 10, (n, 3))
    q = a.astype(f32)
    u, v = (rng.normal(size=(n, 3)) * 0.4).astype(f32), (rng.normal(size=(n, 3)) * 0.4).astype(f32)
    scene = rt.Scene.build("test_sphere", 1.0)
    fresh.upload(scene)
    fresh.set_quads(rt.make_quads(q, u, v, np.ones(n, np.uint8), np.zeros(n, np.uint32)))
    info = fresh.scene_info()
    assert info["n_planar"] == n and info["tree_in_lds"] == 0
    p = rt.make_params(48, 48, 2, max_depth=4, seed=5)
    tree = fresh.render(scene.camera, p)
    walk = fresh.render(scene.camera, rt.make_params(48, 48, 2, max_depth=4, seed=5, flags=f.FLAG_BRUTE_FORCE))
    _same(tree, walk, "tree against list walk")


# ---- 6. validation ------------------------------------------------------------------------------------------------------------------
def test_invalid_sets_are_refused_and_the_previous_set_stays(rt, fresh):
    f = rt._ffi
    scene = rt.Scene.build("sphere_scene", 16 / 9)
    p = rt.make_params(96, 54, 4, max_depth=6, seed=2)
    with pytest.raises(rt.RtError, match=r"\(-?\d+\)"):
        fresh.set_quads(_some_quads(rt))  # before an upload: RT_ERR_STATE
    fresh.upload(scene)
    good = _some_quads(rt)
    fresh.set_quads(good)
    before = fresh.render(scene.camera, p)
    q, u, v, kind, mat = _quad_arrays(good)

    def refused(code, **kw):
        args = dict(q=q.copy(), u=u.copy(), v=v.copy(), kind=kind.copy(), mat=mat.copy())
        args.update(kw)
        with pytest.raises(rt.RtError, match=r"failed \(-%d\)" % code):
            fresh.set_quads(rt.make_quads(args["q"], args["u"], args["v"], args["kind"], args["mat"]))
        _same(before, fresh.render(scene.camera, p), "the previous set stays")
    nan_q = q.copy()
    nan_q[1, 2] = np.nan
    refused(f.ERR_INVALID, q=nan_q)
    inf_u = u.copy()
    inf_u[0, 0] = np.inf
    refused(f.ERR_INVALID, u=inf_u)
    refused(f.ERR_INVALID, kind=np.array([0, 2], np.uint8))
    refused(f.ERR_INVALID, mat=np.array([0, scene.flat.n_materials], np.uint32))
    refused(f.ERR_INVALID, v=np.array([u[0] * 2, v[1]], f32))            # degenerate: v parallel to u
    refused(f.ERR_INVALID, v=np.array([u[0] * 2 + f32([0, 1e-4, 0]), v[1]], f32))  # ill-conditioned: below sin^2 = 2^-20
    refused(f.ERR_INVALID, u=np.zeros((2, 3), f32))
    # motion with quads, in both orders
    with pytest.raises(rt.RtError, match=r"failed \(-%d\)" % f.ERR_UNSUPPORTED):
        fresh.set_motion(rt.make_motion([5], [[0.0, 1.0, 0.0]]))
    _same(before, fresh.render(scene.camera, p), "motion refused: the set stays")
    fresh.set_quads(None)
    fresh.set_motion(rt.make_motion([5], [[0.0, 1.0, 0.0]]))
    moving = fresh.render(scene.camera, p)
    with pytest.raises(rt.RtError, match=r"failed \(-%d\)" % f.ERR_UNSUPPORTED):
        fresh.set_quads(good)
    _same(moving, fresh.render(scene.camera, p), "quads refused: the motion stays")


def test_disney_metal_on_a_planar_primitive_is_unsupported(rt, fresh):
    f = rt._ffi
    scene = rt.Scene.build("pbr_sweep_scene", 16 / 9)
    types = scene.arrays()["mat_type"]
    dm = np.nonzero(types == f.MAT_DISNEY_METAL)[0]
    if len(dm) == 0:
        pytest.fail("pbr_sweep_scene is expected to hold a DisneyMetal material")
    fresh.upload(scene)
    g = _some_quads(rt)
    q, u, v, kind, _ = _quad_arrays(g)
    with pytest.raises(rt.RtError, match=r"failed \(-%d\)" % f.ERR_UNSUPPORTED):
        fresh.set_quads(rt.make_quads(q, u, v, kind, [int(dm[0])] * 2))


def test_multi_set_quads_is_all_or_none(rt):
    f = rt._ffi
    scene = rt.Scene.build("sphere_scene", 16 / 9)
    p = rt.make_params(96, 54, 4, max_depth=6, seed=2)
    m = rt.MultiRenderer([0, 0], copy_gather=True)
    try:
        m.upload(scene)
        good = _some_quads(rt)
        m.set_quads(good)
        before = m.render(scene.camera, p)[0]
        q, u, v, kind, mat = _quad_arrays(good)
        with pytest.raises(rt.RtError, match=r"failed \(-%d\)" % f.ERR_INVALID):
            m.set_quads(rt.make_quads(q, u, u * 2, kind, mat))  # degenerate: refused by the first device, none has changed
        assert np.array_equal(_bits(m.render(scene.camera, p)[0]), _bits(before))
        m.set_quads(None)
        single = rt.Renderer(0)
        try:
            single.upload(scene)
            assert np.array_equal(_bits(m.render(scene.camera, p)[0]), _bits(single.render(scene.camera, p)[0]))
        finally:
            single.close()
    finally:
        m.close()


def test_camera_outside_the_reach_of_the_bound_is_refused(rt, fresh):
    f = rt._ffi
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    grey = s.material(f.MAT_DIFFUSE, tex0=s.constant_tex((0.5, 0.5, 0.5)))
    s.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), grey)  # W = 1: the bound holds for origins within 16
    s.set_camera((0, 0, 15.5), (0, 0, 0), (0, 1, 0), 20.0, 1.0)
    near = s.finish(use_bvh=False)
    s2 = rt.Scene.new()
    s2.set_sky(f.SKY_GRADIENT)
    g2 = s2.material(f.MAT_DIFFUSE, tex0=s2.constant_tex((0.5, 0.5, 0.5)))
    s2.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), g2)
    s2.set_camera((0, 0, 17.0), (0, 0, 0), (0, 1, 0), 20.0, 1.0)
    far = s2.finish(use_bvh=False)
    p = rt.make_params(32, 32, 1, max_depth=2, seed=1)
    fresh.upload(near)
    fresh.set_quads(near.quads)
    fresh.render(near.camera, p)
    with pytest.raises(rt.RtError, match=r"failed \(-%d\)" % f.ERR_UNSUPPORTED):
        fresh.render(far.camera, p)
    fresh.set_quads(None)
    fresh.render(far.camera, p)  # without a set the camera is free
