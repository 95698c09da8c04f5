"""The two references of the pbr.rs BRDFs against each other, without a GPU: the binary32 restatement the GPU tests compare with
(np_ref.family_attenuation, A32) and the float64 one (tests/pbr_ref64.py, A64), on the very rays of tests/test_lights_materials.py
(tests/light_material_cases.py builds them, records and scattered directions included).  This is where the numbers of the conditioning
rule come from: nothing here, and nothing in pbr_ref64's header, has seen a kernel's output."""
import numpy as np
import pytest

import light_material_cases as lmc
import pbr_ref64

SCENES = ("edges", "wrapped", "nested")


@pytest.fixture(scope="module")
def refs(rt, orc):
    return {which: lmc.reference(rt, orc, which) for which in SCENES}


@pytest.mark.parametrize("which", SCENES + ("textured",))
def test_rays_cover_the_cases_and_the_rule_swallows_none(rt, orc, which):
    """per case enough live rays in both branches and on the peak; at most half of a case's rays ill-conditioned with a finite S, 150 or
    more well-conditioned (100 over a texture); at most one in 20 without a colour rule: measured 3 rays of the wrapped and 6 of the
    nested scene, every one a DisneyMetal record that faces away from its ray"""
    R = lmc.reference(rt, orc, which)
    lmc.check_coverage(which, R)
    B = lmc.by_case(R)
    print("%s: %d rays without a colour rule, tags %s" % (which, B["unheld"].sum(), sorted(set(B["type"][B["unheld"]].tolist()))))
    assert B["unheld"].sum() <= 10
    if which in ("wrapped", "nested"):  # records that face away from their ray are held by the ordinary rules: hundreds below the large
        assert (B["inverted"] & ~B["unheld"]).sum() >= (300 if which == "wrapped" else 30)  # rotations, some below the small ones


def _relative(B, sel):
    with np.errstate(all="ignore"):
        a32, a64 = B["A32"][sel].astype(np.float64), B["A64"][sel]
        return np.where(a32 == a64, 0.0, np.abs(a32 - a64) / np.abs(a64))


def test_well_conditioned_rays_agree_to_the_colour_tolerance(refs):
    """S <= S_WELL = 5e-6: A32 within rtol 2e-5 of A64 (the largest difference measured: 1.7e-5)"""
    worst = 0.0
    for which in SCENES:
        B = lmc.by_case(refs[which])
        well = B["well"]
        assert well.sum() > 1000 and np.isfinite(B["A64"][well]).all() and np.isfinite(B["A32"][well]).all(), which
        rel = _relative(B, well)
        print("%s: %d well-conditioned rays, largest relative difference %.3g" % (which, well.sum(), rel.max()))
        worst = max(worst, rel.max())
        assert np.allclose(B["A32"][well], B["A64"][well], rtol=2e-5, atol=0), (which, rel.max())
    print("S_WELL %.1e: largest relative difference of a well-conditioned ray %.3g" % (pbr_ref64.S_WELL, worst))


def test_ill_conditioned_rays_stay_within_f_ref_of_their_conditioning(refs):
    """S > S_WELL: F_ref = max |A32 - A64| / (S |A64|) over every case; measured 4.0 (7.2 on a smaller draw of the same rays), held to
    F_REF = 8, a quarter of what the kernels are given"""
    f_ref = 0.0
    for which in SCENES:
        B = lmc.by_case(refs[which])
        ill = B["ill"]
        fin = np.isfinite(B["A64"][ill]).all(axis=1) & np.isfinite(B["A32"][ill]).all(axis=1) & np.isfinite(B["S"][ill])
        assert ill.sum() > 100 and fin.all(), (which, int(ill.sum()), int((~fin).sum()))
        ratio = (_relative(B, ill).max(axis=1) / B["S"][ill]).max()
        print("%s: %d ill-conditioned rays, F_ref %.3g" % (which, ill.sum(), ratio))
        f_ref = max(f_ref, ratio)
    print("F_ref %.3g, F_REF %.3g, F_GPU %.3g" % (f_ref, pbr_ref64.F_REF, pbr_ref64.F_GPU))
    assert f_ref <= pbr_ref64.F_REF and pbr_ref64.F_GPU == 4.0 * pbr_ref64.F_REF


def test_float64_reference_on_values_worked_by_hand():
    """anchors of pbr_ref64 that need no other code: at normal incidence and exit (n = -rd = dir_o) h = n, every Fresnel power is 0"""
    n = np.array([[1.0, 0.0, 0.0]])  # (off the pole, where Vec3A::Y.cross(on) of the tangent vanishes)
    on, rd, out = n, -n, n
    pi, inv_pi = pbr_ref64.PI, pbr_ref64.FRAC_1_PI
    tex = np.array([0.7, 0.5, 0.3])
    att = lambda ty, p0=0.0, p1=0.0, p2=0.0, t1=(0, 0, 0): pbr_ref64.attenuation(ty, tex, t1, p0, p1, p2, n, on, rd, out)[0]
    assert np.allclose(att(6, 0.0), 2.0 * tex, rtol=1e-15)            # OrenNayar without roughness: Lambert's albedo 2 cos
    assert np.allclose(att(7, 0.6), 2.0 * tex, rtol=1e-15)            # fl = fv = 0: fd = 1
    assert np.allclose(att(9, 0.5, 0.0), 2.0 * tex, rtol=1e-15)       # no subsurface: fd = 1
    assert np.allclose(att(9, 0.5, 1.0), 2.0 * tex * 1.25 * 0.5, rtol=1e-15)  # fss = 1.25 (1 1 (1/2 - 1/2) + 1/2)
    assert np.allclose(att(11, 0.5), 0.0, atol=0)                     # sheen is the Fresnel power alone
    a = 0.25  # DisneyMetal, isotropic branch: D = 1 / (pi a^2) on the peak, G = (1 / 2)^2, F = albedo
    assert np.allclose(att(10, 0.5, -20.0), tex * (1.0 / (pi * a * a)) * 0.25 * 2.0 * pi, rtol=1e-14)
    # the anisotropic branch with aspect 1 (p1 = 0) is the same lobe: ax = ay = a
    assert np.allclose(att(10, 0.5, 0.0, 0.3), att(10, 0.5, -20.0), rtol=1e-12)
    # RoughPlastic at eta = 1: no interface, F = 0, the diffuse colour alone: kd / pi * 2 pi
    assert np.allclose(att(8, 0.3, 1.0, t1=(0.2, 0.6, 0.9)), np.array([0.2, 0.6, 0.9]) * inv_pi * 2.0 * pi, rtol=1e-14)
    # Clearcoat without gloss: a = 0.1, D = (a^2 - 1) / (pi ln(a^2) a^2) on the peak, F = 0.4 (the binary32 0.4), G = 1 / 4
    a2 = float(np.float32(0.1)) ** 2
    assert np.allclose(att(12, 0.0), 0.25 * float(np.float32(0.4)) * (a2 - 1.0) / (pi * np.log(a2) * a2) * 0.25 * 2.0 * pi, rtol=1e-14)


def test_sensitivity_finds_the_peak_and_spares_the_plateau():
    """a sharp lobe (DisneyMetal at alpha_min) moves by far more than S_WELL on its peak and by ulps away from it; a flat one never does"""
    n = np.array([[0.0, 1.0, 0.0]] * 2)
    rd = np.array([[0.6, -0.8, 0.0]] * 2)
    out = np.array([[0.6, 0.8, 0.0], [-0.28, 0.96, 0.0]])  # the mirror direction; 53 degrees from it
    tex = (0.7, 0.5, 0.3)
    S = pbr_ref64.sensitivity(10, tex, tex, 0.0, -20.0, 0.0, n, n, rd, out)
    assert S[0] > 100 * pbr_ref64.S_WELL and S[1] < pbr_ref64.S_WELL, S
    S = pbr_ref64.sensitivity(7, tex, tex, 0.6, 0.0, 0.0, n, n, rd, out)
    assert (S < pbr_ref64.S_WELL).all(), S
