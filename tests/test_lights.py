"""Light importance sampling on the GPU (rt_set_lights).  Frames without a set do not move by one bit; single rays equal the numpy
restatement (tests/light_ref.py) under every flag; the analytic anchor (Lambert's polygon form factor) shows the estimator unbiased and
less noisy; every path through the renderer agrees bit for bit with a set; lens and planar sets combine, motion is refused; invalid
sets are refused and the previous set stays."""
import numpy as np
import pytest

import lens_ref
import light_ref
import quad_ref
from helpers import path_keys

pytestmark = pytest.mark.gpu
f32 = np.float32
np_ref = quad_ref.np_ref
FLT_MAX = np.finfo(f32).max


def _bits(a):
    """the bit patterns of an array: uint32 for the 4-byte types (a NaN equals itself, -0 differs from 0), bytes for `alive`"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same(a, b, what=""):
    assert np.array_equal(_bits(a[0]), _bits(b[0])), what
    assert a[2].n_rays == b[2].n_rays and list(a[2].rays_per_depth) == list(b[2].rays_per_depth), what


@pytest.fixture
def fresh(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


def _light_arrays(lights):
    n = lights.n
    return tuple(np.ctypeslib.as_array(p, shape=(3 * n,)).reshape(n, 3).astype(f32) for p in (lights.q, lights.u, lights.v))


# ---- 1. frames without a set do not move ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nx,ny,spp,scale,at", [("sphere_scene", 160, 90, 8, 1.0, (0, 3, 0)), ("cornell_box", 96, 96, 8, 100.0, (213, 554, 227))])
def test_frames_without_a_set_do_not_move(rt, fresh, name, nx, ny, spp, scale, at):
    scene = rt.Scene.build(name, nx / ny)
    p = rt.make_params(nx, ny, spp, max_depth=12, seed=7)
    fresh.upload(scene)
    never = fresh.render(scene.camera, p)
    lights = rt.make_lights([at], [[scale, 0, 0]], [[0, 0, scale]])
    fresh.set_lights(lights)
    with_set = fresh.render(scene.camera, p)
    if name == "cornell_box":
        assert not np.array_equal(_bits(with_set[0]), _bits(never[0])), "the set must change the samples"
    fresh.set_lights(None)
    _same(never, fresh.render(scene.camera, p), "set, then cleared with NULL")
    fresh.set_lights(lights)
    fresh.upload(scene)  # an upload clears the set
    _same(never, fresh.render(scene.camera, p), "an upload clears the set")


# ---- 2. single rays ---------------------------------------------------------------------------------------------------------------
MATS = [{"type": 1, "tex": (0.7, 0.3, 0.2)}, {"type": 2, "tex": (0.4, 0.6, 0.8)}, {"type": 7, "tex": (0.8, 0.7, 0.3), "p0": 0.6},
        {"type": 3, "color": (0.8, 0.7, 0.6), "p0": 0.1}, {"type": 0, "tex": (5.0, 5.0, 5.0)}]
SPHERES = [((-2.0, 0.8, 0.5), 0.8, 1), ((0.3, 0.9, -1.5), 0.9, 2), ((2.2, 0.7, 0.8), 0.7, 3)]  # Lambert, BurleyDiffuse, Metal
FLOOR = ((-5.0, 0.0, -5.0), (10.0, 0.0, 0.0), (0.0, 0.0, 10.0), 0)   # Q, u, v, material: y = 0
EMITTER = ((-1.0, 4.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), 4)   # y = 4
# the emitter; a larger quad above it that overlaps it as seen from the floor; one below the floor plane
LIGHTS3 = ([[-1.0, 4.0, -1.0], [-0.5, 5.0, -1.5], [-1.0, -2.0, -1.0]], [[2.0, 0, 0], [3.0, 0, 0.2], [2.0, 0, 0]], [[0, 0, 2.0], [0, 0.3, 2.5], [0, 0, 2.0]])
DEPTHS = (0, 1, 7)


def _single_scene(rt, planar):
    """floor and emitter as axis-aligned rectangles, or (planar) as quads of the planar set"""
    f = rt._ffi
    s = rt.Scene.new()
    s.set_sky(f.SKY_GRADIENT)
    mats = [s.material(f.MAT_DIFFUSE, tex0=s.constant_tex(MATS[0]["tex"])), s.material(f.MAT_LAMBERT, tex0=s.constant_tex(MATS[1]["tex"])),
            s.material(f.MAT_BURLEY_DIFFUSE, tex0=s.constant_tex(MATS[2]["tex"]), p=(0.6,)), s.material(f.MAT_METAL, color=MATS[3]["color"], p=(0.1,)),
            s.material(f.MAT_EMISSION, tex0=s.constant_tex(MATS[4]["tex"]))]
    for k, (c, r, m) in enumerate(SPHERES):
        s.sphere(c, r, mats[m], "s%d" % k)
    for Q, u, v, m in (FLOOR, EMITTER):
        if planar:
            s.quad(Q, u, v, mats[m])
        else:
            s.rect(f.RECT_XZ, Q, tuple(np.add(np.add(Q, u), v)), mats[m])
    s.set_camera((0, 3, 12), (0, 1, 0), (0, 1, 0), 40.0, 1.0)
    return s.finish(use_bvh=False)


def _rays(m, seed):
    """from above and from the sides at the floor and the three spheres"""
    rng = np.random.default_rng(seed)
    which = rng.integers(0, 4, m)
    tgt = np.stack([rng.uniform(-4, 4, m), np.zeros(m), rng.uniform(-4, 4, m)], axis=1)
    for k, (c, r, _) in enumerate(SPHERES):
        sel = which == k + 1
        tgt[sel] = np.array(c) + rng.normal(size=(sel.sum(), 3)) * r * 0.45
    org = np.stack([rng.uniform(-6, 6, m), rng.uniform(1.5, 3.5, m), rng.uniform(-6, 6, m)], axis=1)
    d = tgt - org
    d /= np.linalg.norm(d, axis=1)[:, None]
    return org.astype(f32), d.astype(f32)


def _expected(planar, L, o, d, keys, depth):
    """hit, t and the scatter of tests/light_ref.py for every ray (entry order: spheres, then floor and emitter)"""
    m = len(o)
    ns = len(SPHERES)
    want = {"hit": np.full(m, -1, np.int32), "t": np.zeros(m, f32), "alive": np.zeros(m, np.uint8), "o": np.zeros((m, 3), f32),
            "d": np.zeros((m, 3), f32), "attenuation": np.zeros((m, 3), f32)}
    info = [None] * m
    mat_of = np.full(m, -1)
    flats = (FLOOR, EMITTER)
    fq, fu, fv = (np.array([x[i] for x in flats], f32) for i in range(3))
    normal, _, _ = quad_ref.setup(fq, fu, fv)
    for k in range(m):
        ok, dk = tuple(f32(x) for x in o[k]), tuple(f32(x) for x in d[k])
        t_max, hit, rec = f32(FLT_MAX), -1, None
        for s_, (c, r, _) in enumerate(SPHERES):
            h = np_ref.sphere_hit(np_ref.v3(*c), f32(r), ok, dk, f32(1e-3), t_max)
            if h is not None:
                hit, t_max, rec = s_, f32(h["t"]), h
        if planar:
            ph, pt, al, be = quad_ref.closest(fq, fu, fv, [0, 0], o[k:k + 1], d[k:k + 1], base=ns, t0=[t_max], hit0=[hit])
            if ph[0] >= ns:
                hit, t_max = int(ph[0]), f32(pt[0])
                rec = quad_ref.hit_record(normal[hit - ns], o[k], d[k], pt[0], al[0], be[0])
        else:
            for j, (Q, u, v, _) in enumerate(flats):
                h = np_ref.rect_hit(1, np_ref.v3(*Q), np_ref.v3(*np.add(np.add(Q, u), v)), ok, dk, f32(1e-3), t_max)
                if h is not None and not np.isnan(h["t"]):
                    hit, t_max, rec = ns + j, f32(h["t"]), h
        if hit < 0:
            continue
        mm = MATS[SPHERES[hit][2] if hit < ns else flats[hit - ns][3]]
        mat_of[k] = mm["type"]
        want["hit"][k], want["t"][k] = hit, t_max
        alive, att, so, sd, _, info[k] = light_ref.scatter(mm, dk, rec, np_ref.Rng(int(keys[k][0]), int(keys[k][1]), depth), L)
        if alive:
            want["alive"][k], want["o"][k], want["d"][k], want["attenuation"][k] = 1, so, sd, att
    return want, info, mat_of


_CACHE = {}


def _single_expected(planar):
    if planar in _CACHE:
        return _CACHE[planar]
    m = 1344  # per depth: 4 032 rays in all
    L = light_ref.setup(*LIGHTS3)
    per_depth = []
    for depth in DEPTHS:
        o, d = _rays(m, 100 + depth)
        keys = path_keys(0, np.arange(m), np.zeros(m, np.int64))  # (the production path derives slot i's key: seed 0, pixel i, sample 0)
        want, info, mat_of = _expected(planar, L, o, d, keys, depth)
        per_depth.append(dict(o=o, d=d, keys=keys, depth=depth, want=want, info=info, mat_of=mat_of))
    # the rays cover the ground, shown on the restatement's side alone
    infos = [i for X in per_depth for i in X["info"] if i is not None and i["branch"] is not None]
    own = [i for i in infos if i["branch"] == "own"]
    light = [i for i in infos if i["branch"] == "light"]
    assert len(own) >= len(infos) // 4 and len(light) >= len(infos) // 4 and len(infos) > 2000
    assert any(not (i["c"] > 0) for i in light), "a light-chosen direction below the horizon"
    assert any(i["p_L"] > 0 for i in own), "a hemisphere-chosen direction with p_L > 0"
    assert any(i["n_contrib"] >= 2 for i in infos), "two lights contribute to p_L"
    for ty in (1, 2, 7, 3):
        assert sum(int((X["mat_of"] == ty).sum()) for X in per_depth) > 300, ty
    _CACHE[planar] = per_depth
    return per_depth


def _check_rays(got, X, what):
    want, mat_of = X["want"], X["mat_of"]
    assert np.array_equal(got["hit"], want["hit"]), (what, int((got["hit"] != want["hit"]).sum()))
    assert np.array_equal(_bits(got["t"]), _bits(want["t"])), what
    assert np.array_equal(got["alive"], want["alive"]), (what, int((got["alive"] != want["alive"]).sum()), np.nonzero(got["alive"] != want["alive"])[0][:5])
    live = want["alive"] == 1
    for key in ("o", "d"):
        bad = (_bits(got[key]) != _bits(want[key])).any(axis=1) & live
        assert not bad.any(), (what, key, int(bad.sum()), np.nonzero(bad)[0][:5], mat_of[bad][:5])
    exact = live & np.isin(mat_of, (1, 2, 3))  # Diffuse and Lambert over constant textures (and Metal): bit for bit
    bad = (_bits(got["attenuation"]) != _bits(want["attenuation"])).any(axis=1) & exact
    assert not bad.any(), (what, "attenuation", int(bad.sum()), np.nonzero(bad)[0][:5], mat_of[bad][:5])
    pbr = live & (mat_of == 7)  # the project's colour tolerance for the pbr.rs materials
    assert np.allclose(got["attenuation"][pbr], want["attenuation"][pbr], rtol=2e-5, atol=0), what


def _flag_sets(rt):
    f = rt._ffi
    return {"0": 0, "brute": f.FLAG_BRUTE_FORCE, "production": f.FLAG_PRODUCTION_KERNELS, "both": f.FLAG_BRUTE_FORCE | f.FLAG_PRODUCTION_KERNELS}


@pytest.mark.parametrize("planar", [False, True], ids=["rects", "with_set_quads"])
@pytest.mark.parametrize("flags", ["0", "brute", "production", "both"])
def test_single_rays_equal_the_restatement(rt, fresh, flags, planar):
    """(planar: test 5's combination with rt_set_quads — a Diffuse quad floor and an emissive quad in the planar set)"""
    fl = _flag_sets(rt)[flags]
    per_depth = _single_expected(planar)
    scene = _single_scene(rt, planar)
    fresh.upload(scene)
    if planar:
        fresh.set_quads(scene.quads)
    for X in per_depth:
        fresh.set_lights(None)
        plain = fresh.debug_bounce(X["o"], X["d"], X["keys"], depth=X["depth"], flags=fl)
        fresh.set_lights(rt.make_lights(*LIGHTS3))
        got = fresh.debug_bounce(X["o"], X["d"], X["keys"], depth=X["depth"], flags=fl)
        _check_rays(got, X, "depth %d" % X["depth"])
        metal = X["mat_of"] == 3  # Metal rays: every output equals the same call without a set
        assert metal.sum() > 100
        for key in ("hit", "t", "alive", "o", "d", "attenuation", "radiance"):
            assert np.array_equal(_bits(got[key][metal]), _bits(plain[key][metal])), key


@pytest.mark.parametrize("n", [1, 16])
def test_single_rays_with_one_and_sixteen_lights(rt, fresh, n):
    rng = np.random.default_rng(n)
    q = np.concatenate([f32([[-1.0, 4.0, -1.0]]), rng.uniform(-4, 4, (n - 1, 3)).astype(f32) + f32([0, 4, 0])])
    u = np.concatenate([f32([[2.0, 0, 0]]), rng.normal(size=(n - 1, 3)).astype(f32)])
    v = np.concatenate([f32([[0, 0, 2.0]]), rng.normal(size=(n - 1, 3)).astype(f32)])
    L = light_ref.setup(q, u, v)
    X = _single_expected(False)[1]
    sub = slice(0, 256)
    want, info, mat_of = _expected(False, L, X["o"][sub], X["d"][sub], X["keys"][sub], X["depth"])
    assert sum(1 for i in info if i is not None and i["branch"] == "light") > 40
    scene = _single_scene(rt, False)
    fresh.upload(scene)
    fresh.set_lights(rt.make_lights(q, u, v))
    for fl in _flag_sets(rt).values():
        got = fresh.debug_bounce(X["o"][sub], X["d"][sub], X["keys"][sub], depth=X["depth"], flags=fl)
        _check_rays(got, dict(want=want, mat_of=mat_of), "n = %d, flags %d" % (n, fl))


# ---- 3. the analytic anchor -------------------------------------------------------------------------------------------------------
def _form_factor(x, normal, corners):
    """Lambert's edge sum in float64: (1 / 2 pi) sum theta_i n . (r_i x r_{i+1}) / |r_i x r_{i+1}|"""
    r = [np.asarray(c, np.float64) - x for c in corners]
    r = [v / np.linalg.norm(v) for v in r]
    total = 0.0
    for i in range(len(r)):
        a, b = r[i], r[(i + 1) % len(r)]
        g = np.cross(a, b)
        total += np.arccos(np.clip(np.dot(a, b), -1.0, 1.0)) * np.dot(normal, g) / np.linalg.norm(g)
    return abs(total) / (2.0 * np.pi)


@pytest.mark.parametrize("floor", ["diffuse", "lambert"])
def test_analytic_anchor_unbiased_and_less_noisy(rt, fresh, floor):
    f = rt._ffi
    albedo, Le = 0.5, 8.0
    Q, u, v = (1.0, 3.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)  # the emitter: 1 x 1 at height 3, beside the camera's axis
    s = rt.Scene.new()
    s.set_sky(f.SKY_BLACK)
    grey = s.material(f.MAT_DIFFUSE if floor == "diffuse" else f.MAT_LAMBERT, tex0=s.constant_tex((albedo,) * 3))
    s.quad((-50.0, 0.0, -50.0), (100.0, 0.0, 0.0), (0.0, 0.0, 100.0), grey)
    s.quad(Q, u, v, s.material(f.MAT_EMISSION, tex0=s.constant_tex((Le,) * 3)))
    s.set_camera((0, 10, 0), (0, 0, 0), (0, 0, 1), 0.01, 1.0)
    scene = s.finish()
    corners = [np.array(Q, np.float64) + a * np.array(u) + b * np.array(v) for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))]
    F = _form_factor(np.zeros(3), np.array([0.0, 1.0, 0.0]), corners)
    assert 0.005 <= F <= 0.05 and min(c[1] for c in corners) > 0
    truth = albedo * Le * F
    fresh.upload(scene)
    fresh.set_quads(scene.quads)

    def pixels(spp):
        img = fresh.render(scene.camera, rt.make_params(8, 8, spp, max_depth=1, seed=3))[0]
        assert np.array_equal(img[..., 0], img[..., 1]) and np.array_equal(img[..., 0], img[..., 2])
        px = img[..., 0].astype(np.float64).ravel()
        return px.mean(), px.std(ddof=1) / 8.0, px.var(ddof=1)
    lights = scene.lights
    assert lights.n == 1
    fresh.set_lights(lights)
    m, sd, var_with = pixels(4096)
    print("with the set: mean %.6f truth %.6f s %.6f" % (m, truth, sd))
    assert abs(m - truth) <= 6 * sd and sd <= 0.01 * m, (m, truth, sd)
    fresh.set_lights(None)
    # without: a sample is nonzero with probability about F, so s / m = sqrt((1 - F) / F) / (8 sqrt(spp)) <= 0.01 needs
    # spp >= (1 - F) / (0.0064 F); the measured s of 64 pixels scatters by 9 %, hence half as many again, then the next power of two
    spp0 = 1 << int(np.ceil(np.log2(1.5 * (1.0 - F) / (0.0064 * F))))
    m0, sd0, _ = pixels(spp0)
    print("without, %d spp: mean %.6f truth %.6f s %.6f" % (spp0, m0, truth, sd0))
    assert abs(m0 - truth) <= 6 * sd0 and sd0 <= 0.01 * m0, (m0, truth, sd0)
    _, _, var_without = pixels(4096)
    print("pixel variance at 4096 spp: with %.3e without %.3e" % (var_with, var_without))
    assert var_with <= 0.25 * var_without, (var_with, var_without)


# ---- 4. every path through the renderer agrees ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cornell_box", "spheres"])
def test_every_path_agrees_with_a_set(rt, fresh, which):
    f = rt._ffi
    nx = ny = 64
    spp, depth = 16, 8
    if which == "cornell_box":
        scene = rt.Scene.build("cornell_box", 1.0)
        lights = scene.lights
    else:
        scene, lights = rt.Scene.build("sphere_scene", 1.0), rt.make_lights([[-1.0, 3.0, -1.0]], [[2.0, 0, 0]], [[0, 0, 2.0]])  # one quad in the air

    def render(opts=(), **kw):
        for k, val in opts:
            fresh.set_option(k, val)
        fresh.upload(scene)
        fresh.set_lights(lights)
        out = fresh.render(scene.camera, rt.make_params(nx, ny, spp, max_depth=depth, seed=21, **kw))
        info = fresh.scene_info()
        for k, _ in opts:
            fresh.set_option(k, 0)
        return out, info
    base, info = render()
    fresh.set_lights(None)
    assert not np.array_equal(_bits(fresh.render(scene.camera, rt.make_params(nx, ny, spp, max_depth=depth, seed=21))[0]), _bits(base[0]))
    _same(base, render(flags=f.FLAG_BRUTE_FORCE)[0], "list walk")
    _same(base, render(spp_slice=4)[0], "4 slices")
    for order in (1, 2):
        _same(base, render([("pixel_order", order)])[0], "pixel order %d" % order)
    if which == "spheres":
        assert info["grid"] == 1 and info["general_kernels"] == 0
        _same(base, render([("grid", 1)])[0], "no grid")
        _same(base, render([("primary_lists", 1)])[0], "no candidate lists")
    full = np.zeros_like(base[0])
    for sid in range(3):
        fresh.upload(scene)
        fresh.set_lights(lights)
        part = fresh.render(scene.camera, rt.make_params(nx, ny, spp, max_depth=depth, seed=21, shard_band=8, shard_count=3, shard_id=sid))[0]
        rows = [fresh._lib.rt_shard_row_to_image_row(r, 8, 3, sid) for r in range(part.shape[0])]
        full[rows] = part
    assert np.array_equal(_bits(full), _bits(base[0])), "3 shards"
    m = rt.MultiRenderer([0, 0], copy_gather=True)
    try:
        m.upload(scene)
        m.set_lights(lights)
        assert np.array_equal(_bits(m.render(scene.camera, rt.make_params(nx, ny, spp, max_depth=depth, seed=21))[0]), _bits(base[0])), "two contexts"
    finally:
        m.close()


# ---- 5. combinations --------------------------------------------------------------------------------------------------------------
def test_lens_and_lights_at_depth_0(rt, fresh):
    """primary rays through the thin lens (tests/lens_ref.py) into the single-ray scene; their first bounce equals tests/light_ref.py,
    and the frame's depth-0 LENS x LIGHTS kernels agree with the list walk"""
    scene = _single_scene(rt, False)
    fresh.upload(scene)
    fresh.set_lens((0.3, 9.0))
    fresh.set_lights(rt.make_lights(*LIGHTS3))
    nx = ny = 24
    p = rt.make_params(nx, ny, 1, max_depth=1, seed=9)
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    o, d, keys = lens_ref.lens_rays(scene.camera, p, ii.ravel(), jj.ravel(), np.zeros(nx * ny, np.int64), 0.3, 9.0)
    want, info, mat_of = _expected(False, light_ref.setup(*LIGHTS3), o, d, keys, 0)
    assert (mat_of >= 0).sum() > 100
    got = fresh.debug_bounce(o, d, keys, depth=0)
    _check_rays(got, dict(want=want, mat_of=mat_of), "lens rays")
    pf = rt.make_params(48, 48, 4, max_depth=6, seed=9)
    _same(fresh.render(scene.camera, pf), fresh.render(scene.camera, rt.make_params(48, 48, 4, max_depth=6, seed=9, flags=rt._ffi.FLAG_BRUTE_FORCE)), "lens x lights")


def test_motion_and_lights_refuse_each_other(rt, fresh):
    f = rt._ffi
    scene = rt.Scene.build("sphere_scene", 16 / 9)
    p = rt.make_params(96, 54, 4, max_depth=6, seed=2)
    fresh.upload(scene)
    lights = rt.make_lights([[0, 3, 0]], [[1, 0, 0]], [[0, 0, 1]])
    motion = rt.make_motion([5], [[0.0, 1.0, 0.0]])
    fresh.set_lights(lights)
    before = fresh.render(scene.camera, p)
    with pytest.raises(rt.RtError, match=r"failed \(-%d\)" % f.ERR_UNSUPPORTED):
        fresh.set_motion(motion)
    _same(before, fresh.render(scene.camera, p), "motion refused: the set stays")
    fresh.set_lights(None)
    fresh.set_motion(motion)
    moving = fresh.render(scene.camera, p)
    with pytest.raises(rt.RtError, match=r"failed \(-%d\)" % f.ERR_UNSUPPORTED):
        fresh.set_lights(lights)
    _same(moving, fresh.render(scene.camera, p), "lights refused: the motion stays")


# ---- 6. validation ----------------------------------------------------------------------------------------------------------------
def test_invalid_sets_are_refused_and_the_previous_set_stays(rt, fresh):
    f = rt._ffi
    scene = rt.Scene.build("cornell_box", 1.0)
    p = rt.make_params(64, 64, 4, max_depth=6, seed=2)
    good = scene.lights
    with pytest.raises(rt.RtError, match=r"failed \(-%d\)" % f.ERR_STATE):
        fresh.set_lights(good)  # before an upload
    fresh.upload(scene)
    fresh.set_lights(good)
    before = fresh.render(scene.camera, p)
    q, u, v = _light_arrays(good)

    def refused(**kw):
        args = dict(q=q.copy(), u=u.copy(), v=v.copy())
        args.update(kw)
        with pytest.raises(rt.RtError, match=r"failed \(-%d\)" % f.ERR_INVALID):
            fresh.set_lights(rt.make_lights(args["q"], args["u"], args["v"]))
        _same(before, fresh.render(scene.camera, p), "the previous set stays")
    refused(q=np.tile(q, (17, 1)), u=np.tile(u, (17, 1)), v=np.tile(v, (17, 1)))
    for name in ("q", "u", "v"):
        for bad in (np.nan, np.inf):
            a = dict(q=q, u=u, v=v)[name].copy()
            a[0, 1] = bad
            refused(**{name: a})
    refused(v=u * 2)  # u parallel to v
    # conditioning: |u x v|^2 >= 2^-20 |u|^2 |v|^2, i.e. sin >= 2^-10, evaluated in double on the f32 inputs
    uu = f32([[1.0, 0.0, 0.0]])

    def sin2(vv):
        a, b = uu[0].astype(np.float64), vv[0].astype(np.float64)
        return np.dot(np.cross(a, b), np.cross(a, b)) / (np.dot(a, a) * np.dot(b, b))
    below, above = f32([[1.0, 2.0 ** -10 * 0.999, 0.0]]), f32([[1.0, 2.0 ** -10 * 1.001, 0.0]])
    assert sin2(below) < f.PLANAR_MIN_SIN2 < sin2(above)
    refused(u=uu, v=below)
    fresh.set_lights(rt.make_lights(q, uu, above))  # just above the limit: accepted
    fresh.set_lights(rt.make_lights(np.tile(q, (16, 1)), np.tile(u, (16, 1)), np.tile(v, (16, 1))))  # 16 lights: accepted


def test_multi_set_lights_is_all_or_none(rt):
    f = rt._ffi
    scene = rt.Scene.build("cornell_box", 1.0)
    p = rt.make_params(64, 64, 4, max_depth=6, seed=2)
    m = rt.MultiRenderer([0, 0], copy_gather=True)
    try:
        m.upload(scene)
        m.set_lights(scene.lights)
        before = m.render(scene.camera, p)[0]
        q, u, v = _light_arrays(scene.lights)
        with pytest.raises(rt.RtError, match=r"failed \(-%d\)" % f.ERR_INVALID):
            m.set_lights(rt.make_lights(q, u, u * 2))  # refused by the first device, none has changed
        assert np.array_equal(_bits(m.render(scene.camera, p)[0]), _bits(before))
    finally:
        m.close()
