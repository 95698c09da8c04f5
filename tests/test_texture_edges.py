"""Texture and sky lookups on the GPU at their edges, held to the exact texel (tests/uv_ref.py; the same scenes and rays as
tests/test_uv_ref_host.py, which holds the reference against the oracle and the ray groups to their coverage conditions).

Every case goes through four paths — k_debug_bounce with the tree in LDS, with tree_placement = 1, the list walk (FLAG_BRUTE_FORCE) and the
kernels of a frame (FLAG_PRODUCTION_KERNELS) — and for every ray `hit` and `t` equal the oracle's bit for bit, the colour is bit for bit a
texel of the ray's candidate set, and a ray with a single candidate returns exactly that texel.  Every scene holds a decoy image in front
of the image under test, so the second image's pool offset is in play; the colours name their texel (uv_ref.make_image, uv_ref.decode).

What the reference inherits and the kernels must keep: at the SOUTH pole the rounded normal has n.y < -1 for a large share of rays, acos is
NaN, the clamp keeps it and the conversion maps it to row 0, the TOP row; a sky direction (0, -nextafter(1, 2), 0) passes the near-one
window and reads the zenith row the same way; at the seam the sign of a zero z picks column 0 or W - 1."""
import numpy as np
import pytest

import texture_edge_cases as tc
import uv_ref
from helpers import primary_rays

pytestmark = pytest.mark.gpu
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _paths(rt, renderer, X):
    """(name, rt_debug_bounce's result, production) for the four paths; the scene's set (motion or quads) is applied after every upload"""
    f = rt._ffi

    def upload(placement):
        renderer.set_option("tree_placement", placement)
        renderer.upload(X["scene"])
        if X.get("motion") is not None:
            renderer.set_motion(X["motion"])
        if X.get("quads") is not None:
            renderer.set_quads(X["quads"])
        assert renderer.scene_info()["tree_in_lds"] == 1 - placement

    def run(flags):
        return renderer.debug_bounce(X["o"], X["d"], X["keys"], depth=tc.DEPTH, flags=flags)
    upload(0)
    yield "tree in LDS", run(0), False
    yield "list walk", run(f.FLAG_BRUTE_FORCE), False
    yield "production kernels", run(f.FLAG_PRODUCTION_KERNELS), True
    upload(1)
    yield "tree in L2", run(0), False
    renderer.set_option("tree_placement", 0)


def _check_hits(got, want_hit, want_t, what):
    assert np.array_equal(got["hit"], want_hit), (what, "hit", int((got["hit"] != want_hit).sum()), np.nonzero(got["hit"] != want_hit)[0][:5])
    k = want_hit >= 0
    assert np.array_equal(_bits(got["t"])[k], _bits(want_t)[k]), (what, "t")


def _check_texels(colour, sel, cand, X, what, squared=False):
    """colour [n, 3] of the rays `sel`: bit for bit a texel of the image under test, and one of the ray's candidates"""
    i, j = uv_ref.decode(colour, X["w"], X["h"], X["eight_bit"], squared=squared)
    bad = sel & (i < 0)
    assert not bad.any(), (what, "not a texel of the image under test", int(bad.sum()), np.nonzero(bad)[0][:5], colour[bad][:3])
    bad = sel & ~uv_ref.in_set(cand, i, j)
    assert not bad.any(), (what, "a texel outside the candidate set", int(bad.sum()), np.nonzero(bad)[0][:5], i[bad][:5], j[bad][:5],
                           cand["i0"][bad][:5], cand["j0"][bad][:5], "rays with n.y beyond 1 among them:", int(cand["nan_row"][bad].sum()))


def _sphere_reference(orc, X):
    """hit and t of every ray: the oracle's list walk; for the moving sphere (the oracle knows no motion) np_ref's Sphere::hit at the ray's time"""
    if X["motion"] is None:
        c = orc.debug_bounce(X["scene"].flat_ptr, X["o"], X["d"], X["keys"], depth=tc.DEPTH, accel=orc.ACCEL_LIST)
        assert np.array_equal(c["hit"] == X["target"], X["ref_hit"])
        return c
    return {"hit": np.where(X["ref_hit"], X["target"], -1).astype(np.int32), "t": X["ref_t"]}


SPHERE_CASES = [(form, image, uv_ref.GROUPS) for form in tc.BARE for image in tc.IMAGES] + [(form, "7x5", ("random", "pole_south")) for form in tc.WRAPPED]


@pytest.mark.parametrize("form,image,groups", SPHERE_CASES, ids=["%s-%s" % c[:2] for c in SPHERE_CASES])
def test_emitting_spheres(rt, orc, renderer, form, image, groups):
    X = tc.sphere_case(rt, form, image, groups)
    _, cand = tc.group_statistics(X)
    c = _sphere_reference(orc, X)
    k = X["ref_hit"]
    first = None
    try:
        for what, g, production in _paths(rt, renderer, X):
            what = (form, image, what)
            _check_hits(g, c["hit"], c["t"], what)
            assert not g["alive"].any(), what
            _check_texels(g["radiance"], k, cand, X, what)
            assert not g["radiance"][~k].any(), (what, "a black sky")
            first = g if first is None else first
        if X["eight_bit"]:  # the same image through the float4 pool: the same bits
            renderer.set_option("texel_pool", 1)
            renderer.upload(X["scene"])
            p = renderer.debug_bounce(X["o"], X["d"], X["keys"], depth=tc.DEPTH)
            for key in p:
                assert np.array_equal(p[key].view(np.uint8), first[key].view(np.uint8)), (form, image, "texel_pool = 1", key)
    finally:
        renderer.set_option("texel_pool", 0)
        renderer.upload(X["scene"])  # (an upload clears the motion)


def test_a_textured_material_that_scatters(rt, orc, renderer):
    """MAT_DIFFUSE wearing the image (texture_value_inline of k_shade): the attenuation is a candidate texel, the rest is the oracle's"""
    X = tc.sphere_case(rt, "off", "7x5", ("pole_south",), mat="diffuse")
    _, cand = tc.group_statistics(X)
    c = _sphere_reference(orc, X)
    k = X["ref_hit"]
    assert c["alive"][k].all()
    for what, g, production in _paths(rt, renderer, X):
        _check_hits(g, c["hit"], c["t"], what)
        assert np.array_equal(g["alive"], c["alive"]), what
        assert np.array_equal(_bits(g["o"])[k], _bits(c["o"])[k]) and np.array_equal(_bits(g["d"])[k], _bits(c["d"])[k]), what
        _check_texels(g["attenuation"], k, cand, X, what)
        assert not g["radiance"][k].any(), what


@pytest.mark.parametrize("image", ["7x5", "256x128", "1025x513"])
def test_sky_directions(rt, orc, renderer, image):
    X = tc.sky_case(rt, image)
    _, cand = tc.sky_statistics(X)
    every = np.ones(len(X["d"]), bool)
    for what, g, production in _paths(rt, renderer, X):
        assert (g["hit"] < 0).all() and not g["alive"].any(), (image, what)
        _check_texels(g["radiance"], every, cand, X, (image, what), squared=True)


@pytest.mark.parametrize("down", [True, False], ids=["down", "up"])
def test_sky_at_depth_0_of_a_frame(rt, renderer, down):
    """8 x 8 pixels, 1 spp, max_depth 1, the camera looking straight down (up): every pixel is the square of a candidate texel of its own
    primary ray (helpers.primary_rays) — the sky site of k_shade at depth 0"""
    image = "1025x513"
    scene = tc.frame_case(rt, image, down)
    w, h, eight = tc.IMAGES[image]
    p = rt.make_params(8, 8, 1, max_depth=1, seed=11)
    renderer.upload(scene)
    img, _, st = renderer.render(scene.camera, p)
    jj, ii = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    _, d, _ = primary_rays(scene, p, ii.ravel(), jj.ravel(), np.zeros(64, np.int64))
    cand = uv_ref.candidates(d, w, h, sky=True)
    assert (cand["j0"] == (h - 1 if down else 0)).mean() > 0.3 and len(np.unique(cand["i0"])) > 8  # around the pole, not beside it
    X = dict(w=w, h=h, eight_bit=eight)
    _check_texels(img.reshape(-1, 3), np.ones(64, bool), cand, X, ("frame", "down" if down else "up"), squared=True)
    assert st.n_rays == 64


def test_rectangles_box_and_planar_set(rt, orc, renderer):
    """no libm on this route: hit, t and the colour are np_ref.rect_hit + np_ref.image_value and quad_ref, bit for bit — on the borders and
    corners (u, v, alpha, beta of exactly 0 and 1) as inside"""
    X = tc.flat_case(rt)
    tc.flat_statistics(X)
    try:
        for what, g, production in _paths(rt, renderer, X):
            _check_hits(g, X["want_hit"].astype(np.int32), X["want_t"], what)
            assert not g["alive"].any(), what
            bad = (_bits(g["radiance"]) != _bits(X["want_colour"])).any(axis=1)
            assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:5], g["radiance"][bad][:3], X["want_colour"][bad][:3])
    finally:
        renderer.upload(X["scene"])  # (an upload clears the planar set)


@pytest.mark.parametrize("where", ["floor", "1e5", "1e6"])
def test_checker(rt, orc, renderer, where):
    """the sign of sin(10 x) sin(10 y) sin(10 z): a coordinate of exactly +-0 gives a product of +-0, which is NOT negative (a floor at y = 0 is
    one colour; a sign-bit test would not be); arguments of 1e5 .. 1e7 need the whole range reduction.  Decided rays equal the reference."""
    X = tc.checker_case(rt, where)
    tc.checker_statistics(X, where)
    c = orc.debug_bounce(X["scene"].flat_ptr, X["o"], X["d"], X["keys"], depth=tc.DEPTH, accel=orc.ACCEL_LIST)
    k = X["ref_hit"]
    assert np.array_equal(c["hit"] == X["target"], k)
    want = tc.checker_colour(X)
    odd, even = _bits(np.array(tc.ODD, f32)), _bits(np.array(tc.EVEN, f32))
    for what, g, production in _paths(rt, renderer, X):
        _check_hits(g, c["hit"], c["t"], (where, what))
        rad = _bits(g["radiance"])
        bad = k & X["decided"] & (rad != _bits(want)).any(axis=1)
        assert not bad.any(), (where, what, int(bad.sum()), np.nonzero(bad)[0][:5], X["p"][bad][:3])
        assert ((rad == odd).all(axis=1) | (rad == even).all(axis=1))[k].all(), (where, what, "an undecided ray takes either colour, nothing else")
