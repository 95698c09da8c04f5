"""Every material a light set affects (rt_set_lights), on the GPU: Diffuse, Lambert and the seven pbr.rs materials at their parameter edges, below
wrappers (the register chain and the NEST loop, the tree in LDS and behind L2) and over checker, Perlin and image textures, under all four flag
sets.  Scenes, rays and references come from tests/light_material_cases.py; the rays include grazing ones and ones whose mirror direction
leads to a small light, where the sharp lobes sit on their peaks.

hit, t, alive, o and d are held bit for bit for every ray, and so are the colours of Diffuse and Lambert and of the paths a set ends.  The colour of a pbr.rs material is
held to rtol 2e-5 of tests/light_ref.py where it is well conditioned, and where it is not to F_GPU S |A64 wgt| around the float64 value
(tests/pbr_ref64.py: S the conditioning, F_GPU its factor, both from the references alone; wgt the light weight of tests/light_ref.py,
whose arithmetic Diffuse and Lambert hold bit for bit).  The few rays below a rotation where the binary32 restatement itself leaves that
rule (`unheld` of tests/light_material_cases.py, 9 rays in all) have no colour rule; every other ray keeps the finiteness check too."""
import numpy as np
import pytest

import light_material_cases as lmc
import pbr_ref64

pytestmark = pytest.mark.gpu
f32 = np.float32
FLAGS = ["0", "brute", "production", "both"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


@pytest.fixture
def fresh(rt):
    r = rt.Renderer(0)
    yield r
    r.close()


def _flag(rt, name):
    f = rt._ffi
    return {"0": 0, "brute": f.FLAG_BRUTE_FORCE, "production": f.FLAG_PRODUCTION_KERNELS, "both": f.FLAG_BRUTE_FORCE | f.FLAG_PRODUCTION_KERNELS}[name]


def _rows(bad):
    return int(bad.sum()), np.nonzero(bad)[0][:5]


def _check(got, plain, X, what, textured=False, production=False):
    want, ty = X["want"], X["type"]
    assert np.array_equal(got["hit"], want["hit"]), (what, "hit") + _rows(got["hit"] != want["hit"])
    assert np.array_equal(_bits(got["t"]), _bits(want["t"])), (what, "t")
    assert np.array_equal(got["alive"], want["alive"]), (what, "alive") + _rows(got["alive"] != want["alive"]) + (ty[got["alive"] != want["alive"]][:5],)
    alive = want["alive"] == 1
    for key in ("o", "d"):
        bad = (_bits(got[key]) != _bits(want[key])).any(axis=1) & alive
        assert not bad.any(), (what, key) + _rows(bad) + (ty[bad][:5], X["chain"][bad][:5])
    dead = X["dead"]  # an affected ray that ends (a light-chosen direction below the horizon): no light, and the colour scatter leaves
    assert dead.sum() >= 20 and not got["radiance"][dead].any(), (what, "radiance of ended paths")
    if not production:  # (the production kernels keep an attenuation for survivors only)
        bad = (_bits(got["attenuation"]) != _bits(X["dead_att"])).any(axis=1) & dead
        assert not bad.any(), (what, "colour of ended paths") + _rows(bad) + (ty[bad][:5],)
    live = X["live"]  # the live rays of the affected materials
    g, w = got["attenuation"].astype(np.float64), want["attenuation"].astype(np.float64)
    with np.errstate(all="ignore"):
        rel = np.where(g == w, 0.0, np.abs(g - w) / np.abs(w)).max(axis=1)
    held = live & ~X["unheld"]
    bad = (np.isfinite(g) != np.isfinite(w)).any(axis=1) & held
    assert not bad.any(), (what, "finiteness") + _rows(bad) + (ty[bad][:5],)
    exact = live & np.isin(ty, (1, 2))
    if textured:  # the texture's value is the oracle's: the oracle's colour tolerance
        assert np.allclose(g[exact], w[exact], rtol=2e-5, atol=1e-6), (what, "Diffuse and Lambert over a texture", rel[exact].max())
    else:
        bad = (_bits(got["attenuation"]) != _bits(want["attenuation"])).any(axis=1) & exact
        assert not bad.any(), (what, "Diffuse and Lambert") + _rows(bad) + (ty[bad][:5],)
    well, ill, unheld = X["well"], X["ill"], X["unheld"] & np.isfinite(w).all(axis=1) & np.isfinite(g).all(axis=1)
    fin = np.isfinite(w).all(axis=1)
    ref = X["A64"] * X["wgt"].astype(np.float64)[:, None]
    bound = pbr_ref64.F_GPU * X["S"][:, None] * np.abs(ref) + ((2e-5 * np.abs(ref) + 1e-6) if textured else 0.0)
    with np.errstate(all="ignore"):
        used = np.where(g == ref, 0.0, np.abs(g - ref) / bound)
    print("%s: well-conditioned %d rays, largest relative difference %.3g; ill-conditioned %d rays, largest share of the bound %.3g; unheld %d rays, "
          "largest relative difference %.3g" % (what, well.sum(), rel[well & fin].max(initial=0.0), ill.sum(), used[ill & fin].max(initial=0.0), X["unheld"].sum(),
                                                rel[unheld].max(initial=0.0)))
    bad = well & fin & ~np.isclose(g, w, rtol=2e-5, atol=1e-6 if textured else 0).all(axis=1)
    assert not bad.any(), (what, "well-conditioned colours") + _rows(bad) + (ty[bad][:5], rel[bad][:5])
    bad = ill & fin & ~(np.abs(g - ref) <= bound).all(axis=1)
    assert not bad.any(), (what, "ill-conditioned colours") + _rows(bad) + (ty[bad][:5], used[bad][:5])
    other = ty == 3  # the Metal ground: every output equals the same call without a set
    assert other.sum() >= 40, what
    for key in ("hit", "t", "alive", "o", "d", "attenuation", "radiance"):
        assert np.array_equal(_bits(got[key][other]), _bits(plain[key][other])), (what, "Metal", key)


def _run(rt, orc, fresh, which, flags, textured=False):
    R = lmc.reference(rt, orc, which)
    lmc.check_coverage(which, R)
    fresh.upload(R["scene"])
    fl = _flag(rt, flags)
    out = []
    for X in R["per_depth"]:
        fresh.set_lights(None)
        plain = fresh.debug_bounce(X["o"], X["d"], X["keys"], depth=X["depth"], flags=fl)
        fresh.set_lights(rt.make_lights(*lmc.LIGHTS))
        got = fresh.debug_bounce(X["o"], X["d"], X["keys"], depth=X["depth"], flags=fl)
        _check(got, plain, X, "%s, %s, depth %d" % (which, flags, X["depth"]), textured, production=flags in ("production", "both"))
        out.append((got, plain, X))
    return out


@pytest.mark.parametrize("flags", FLAGS)
def test_every_affected_material_at_its_parameter_edges(rt, orc, fresh, flags):
    _run(rt, orc, fresh, "edges", flags)


@pytest.mark.parametrize("placement", ["lds", "l2"])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("which", ["wrapped", "nested"])
def test_affected_materials_below_wrappers(rt, orc, fresh, which, flags, placement):
    """po, n and p_L from the world-space record after the chain is unwound, DisneyMetal's tangent from the object-space normal: two wrappers
    in registers, and chains of five and six through the NEST loop"""
    fresh.set_option("tree_placement", 1 if placement == "l2" else 0)
    _run(rt, orc, fresh, which, flags)
    info = fresh.scene_info()
    assert info["nest"] == (1 if which == "nested" else 0) and info["tree_in_lds"] == (0 if placement == "l2" else 1), info


@pytest.mark.parametrize("flags", FLAGS)
def test_textured_materials_under_a_set(rt, orc, fresh, flags):
    """checker, Perlin and image tex0 below Diffuse, Lambert and DisneyDiffuse, an image tex1 below RoughPlastic: the texture's value at the hit
    is the oracle's, from a twin scene that shows it as a Diffuse attenuation; no texture is restated"""
    for got, plain, X in _run(rt, orc, fresh, "textured", flags, textured=True):
        sel = X["live"] & (X["type"] == 1)
        assert sel.sum() >= 100
        # the one multiplication the set adds: the colour without a set (the texture's value on this GPU) times the weight
        lone = (plain["attenuation"][sel] * X["wgt"][sel][:, None]).astype(f32)
        assert np.array_equal(_bits(got["attenuation"][sel]), _bits(lone)), "Diffuse over a texture"
