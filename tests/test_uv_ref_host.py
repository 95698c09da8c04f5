"""The set-valued texel reference (tests/uv_ref.py) against the oracle, without a GPU: for every ray of the scenes of
tests/test_texture_edges.py that the oracle can trace (bare spheres, a negative radius, RotateY and Translate(RotateY), the ENV sky,
rectangles, a box, the checker) the texel the oracle reads lies in the candidate set — and the ray groups meet their coverage conditions on
the reference alone, so that the GPU test cannot pass by leaving the edges out:

  random      at most 0.5 % of the hits have more than one candidate (per image size); at least 95 % of the texels of the 7 x 5 image are read
  pole_south  at most 0.5 %; at least 5 % of the hits have n.y < -1 (acos is NaN: row 0), at least 5 % read row H - 1
  pole_north  at most 0.5 %; at least 5 % of the hits have n.y > 1
  seam        at most 0.5 %; both column 0 and column W - 1 are read
  border      exempt from the cap: at least 20 % ambiguous (images with borders in both directions), decided rays on both sides of a border

The moving sphere has no oracle (it knows no motion): its conditions are held here, its rays on the GPU.  The planar set is quad_ref's."""
import numpy as np
import pytest

import texture_edge_cases as tc
import uv_ref

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _oracle(orc, X):
    return orc.debug_bounce(X["scene"].flat_ptr, X["o"], X["d"], X["keys"], depth=tc.DEPTH, accel=orc.ACCEL_LIST)


def _print(title, stats):
    for g, st in stats.items():
        print("%-28s %-11s %s" % (title, g, "  ".join("%s %s" % (k, ("%.4f" % v) if isinstance(v, float) else v) for k, v in st.items())))


SPHERE_CASES = [(form, image, uv_ref.GROUPS) for form in tc.BARE for image in tc.IMAGES] + [(form, "7x5", ("random", "pole_south")) for form in tc.WRAPPED]


@pytest.mark.parametrize("form,image,groups", SPHERE_CASES, ids=["%s-%s" % c[:2] for c in SPHERE_CASES])
def test_spheres(rt, orc, form, image, groups):
    X = tc.sphere_case(rt, form, image, groups)
    tc.spot_check_against_np_ref(X)
    stats, cand = tc.group_statistics(X)
    _print("%s %s" % (form, image), stats)
    if form == "moving":
        return
    c = _oracle(orc, X)
    k = X["ref_hit"]
    assert np.array_equal(c["hit"] == X["target"], k)
    assert np.array_equal(_bits(c["t"])[k], _bits(X["ref_t"])[k])
    i, j = uv_ref.decode(c["radiance"], X["w"], X["h"], X["eight_bit"])
    assert (i[k] >= 0).all(), "the oracle's colour is a texel of the image under test"
    ok = uv_ref.in_set(cand, i, j)
    assert ok[k].all(), (form, image, int((~ok[k]).sum()), np.nonzero(~ok & k)[0][:5])


def test_a_texture_that_scatters(rt, orc):
    X = tc.sphere_case(rt, "off", "7x5", ("pole_south",), mat="diffuse")
    stats, cand = tc.group_statistics(X)
    _print("diffuse off 7x5", stats)
    c = _oracle(orc, X)
    k = X["ref_hit"]
    assert np.array_equal(c["hit"] == X["target"], k) and c["alive"][k].all()
    i, j = uv_ref.decode(c["attenuation"], X["w"], X["h"], X["eight_bit"])
    assert (i[k] >= 0).all() and uv_ref.in_set(cand, i, j)[k].all()


@pytest.mark.parametrize("image", ["7x5", "256x128", "1025x513"])
def test_sky(rt, orc, image):
    X = tc.sky_case(rt, image)
    stats, cand = tc.sky_statistics(X)
    _print("sky %s" % image, stats)
    c = _oracle(orc, X)
    assert (c["hit"] < 0).all()
    i, j = uv_ref.decode(c["radiance"], X["w"], X["h"], X["eight_bit"], squared=True)
    assert (i >= 0).all(), "the oracle's radiance is the square of a texel of the image under test"
    ok = uv_ref.in_set(cand, i, j)
    assert ok.all(), (image, int((~ok).sum()), np.nonzero(~ok)[0][:5])


def test_rectangles_box_and_planar_set(rt, orc):
    X = tc.flat_case(rt)
    print("rect, box, planar", tc.flat_statistics(X))
    tc.spot_check_flat_against_np_ref(X)
    c = _oracle(orc, X)  # (the oracle knows no planar set: its rays are quad_ref's alone)
    k = X["want_hit"] < X["base"]
    assert np.array_equal(c["hit"][k], X["want_hit"][k])
    h = k & (X["want_hit"] >= 0)
    assert np.array_equal(_bits(c["t"])[h], _bits(X["want_t"])[h])
    assert np.array_equal(_bits(c["radiance"])[h], _bits(X["want_colour"])[h])


@pytest.mark.parametrize("where", ["floor", "1e5", "1e6"])
def test_checker(rt, orc, where):
    X = tc.checker_case(rt, where)
    print("checker %s" % where, tc.checker_statistics(X, where))
    c = _oracle(orc, X)
    k = X["ref_hit"]
    assert np.array_equal(c["hit"] == X["target"], k)
    assert np.array_equal(_bits(c["t"])[k], _bits(X["ref_t"])[k])
    sel = k & X["decided"]
    assert np.array_equal(_bits(c["radiance"])[sel], _bits(tc.checker_colour(X))[sel])


def test_candidates_of_hand_made_normals():
    """the chain itself, on inputs whose answer is known: the poles, the NaN row, the seam with either zero, u = 1 -> column W - 1"""
    n = np.array([[0, -1, 0], [0, 1, 0], [0, -np.nextafter(f32(1), f32(2)), 0], [0, np.nextafter(f32(1), f32(2)), 0], [-1, 0, 0.0], [-1, 0, -0.0], [1, 0, 0]], f32)
    for w, h in ((7, 5), (1, 1), (1025, 513)):
        c = uv_ref.candidates(n, w, h)
        assert c["single"].all()
        assert list(c["j0"]) == [h - 1, 0, 0, 0, h // 2, h // 2, h // 2] and list(c["nan_row"]) == [False, False, True, True, False, False, False]
        assert list(c["i0"][4:]) == [0, w - 1, w // 2]  # atan2(-0, -1) = -pi: u = 0; atan2(+0, -1) = pi: u = 1 -> W, held by the min
        s = uv_ref.candidates(n, w, h, sky=True)
        assert list(s["i0"][4:6]) == [w - 1, 0]
    # texel borders: on even sizes the equator is a row border (v = 1/2) and n = -z a column border (u = 3/4): both neighbours are candidates;
    # n = +x is not (u = 1/2, but atan2 is within 6 ulp of ZERO there, and adding PI swallows that)
    c = uv_ref.candidates(np.array([[1, 0, 0], [0, 0, -1]], f32), 256, 128)
    assert not c["single"].any() and [set(x) for x in c["I"]] == [{128}, {191, 192}] and [set(x) for x in c["J"]] == [{63, 64}] * 2
    img = uv_ref.make_image(7, 5, False)
    i, j = uv_ref.decode(img.reshape(-1, 3), 7, 5, False)
    assert np.array_equal(i, np.tile(np.arange(7), 5)) and np.array_equal(j, np.repeat(np.arange(5), 7))
    assert (uv_ref.decode(uv_ref.make_image(5, 3, False, decoy=True).reshape(-1, 3), 7, 5, False)[0] == -1).all()
    assert (uv_ref.decode(uv_ref.make_image(5, 3, True, decoy=True).reshape(-1, 3), 256, 128, True)[0] == -1).all()
    sq = (uv_ref.make_image(1025, 513, False) ** 2).astype(f32)
    i, j = uv_ref.decode(sq[::37, ::41].reshape(-1, 3), 1025, 513, False, squared=True)
    assert (i >= 0).all()
