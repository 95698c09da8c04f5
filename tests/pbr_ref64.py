"""The seven pbr.rs BRDFs in plain vectorised numpy float64, written from the reference's pbr.rs, math.rs:79-81, 154-156 and
hitable.rs:37-41, 96 — not derived from tests/golden/np_ref.py.  attenuation() is the value Material::scatter returns for a given
scattered direction, without a light weight.  The constants the kernels hold in binary32 (RT_PI, RT_FRAC_1_PI, 0.9f, alpha_min, ...)
enter as their binary32 values, the parameters p0..p2 as the binary32 values the scene stores; everything computed from them, sin, cos
and ln included, is float64.

sensitivity() is the conditioning of that value in its directions: how far it moves when every component of n, rd and dir_o moves by
up to one binary32 ulp.  A binary32 evaluation cannot be expected to agree with this module more closely than that, so the tests split
their rays by it (tests/test_pbr_ref_host.py, tests/test_lights_materials.py):

    S <= S_WELL         the binary32 restatement (np_ref.family_attenuation) and the kernels are held to rtol 2e-5
    S >  S_WELL         held to |x - A64| <= F S |A64| per component, F = F_REF for the restatement, F_GPU for the kernels

Measured on the references alone (np_ref.family_attenuation against this module, no kernel involved; tests/test_pbr_ref_host.py prints
them), on the rays of tests/light_material_cases.py: with S_WELL = 5e-6, a quarter of the project's colour tolerance, the largest
difference of a well-conditioned ray is 1.7e-5 relative (1.3e-5 among records that face their ray), so the threshold stands as it is; and F_ref, the largest |A32 - A64| / (S |A64|)
of an ill-conditioned ray, is 4.0 (7.2 on a smaller draw of the same generator: S is an estimate from N_PROBES moves and scatters by
about that much), which F_REF = 8 bounds.  F_GPU = 4 F_REF = 32: the kernels' sinf, cosf, logf and powi sequences may differ from
numpy's within the ulp bounds that test_libm_class_functions_are_within_their_ulp_bounds holds, and each such difference is amplified as a
perturbation of an input is.
None of the three numbers was chosen by looking at what a kernel returns."""
import numpy as np

S_WELL = 5e-6
F_REF = 8.0
F_GPU = 4.0 * F_REF
N_PROBES = 8


def _c(x):
    """a constant as the kernels hold it: its binary32 value"""
    return float(np.float32(x))


PI = _c(np.pi)
FRAC_1_PI = _c(1.0 / np.pi)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _unit(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def _lerp(a, b, s):  # math.rs:154-156
    return a + (b - a) * s


def _schlick(u):  # math.rs:79-81
    return (1.0 - u) ** 5


def _gtr1(n_dot_h, a):  # pbr.rs:72-79
    if a >= 1.0:
        return np.full_like(n_dot_h, FRAC_1_PI)
    a2 = a * a
    t = 1.0 + (a2 - 1.0) * n_dot_h * n_dot_h
    return (a2 - 1.0) / (PI * np.log(a2) * t)


def _gtr2(n_dot_h, a):  # pbr.rs:81-85
    a2 = a * a
    t = 1.0 + (a2 - 1.0) * n_dot_h * n_dot_h
    return a2 / (PI * t * t)


def _gtr2_aniso(h, ax, ay):  # pbr.rs:87-89
    q = (h[..., 0] / ax) ** 2 + (h[..., 1] / ay) ** 2 + h[..., 2] * h[..., 2]
    return 1.0 / (PI * ax * ay * q * q)


def _smith_ggx(n_dot_v, alpha):  # pbr.rs:92-96
    a, b = alpha * alpha, n_dot_v * n_dot_v
    return 1.0 / (n_dot_v + np.sqrt(a + b - a * b))


def _smith_ggx_aniso(v, ax, ay):  # pbr.rs:98-100
    return 1.0 / (v[..., 2] + np.sqrt((v[..., 0] * ax) ** 2 + (v[..., 1] * ay) ** 2 + v[..., 2] * v[..., 2]))


def _fresnel_dielectric_2(c, eta):  # pbr.rs:107-129
    t2 = 1.0 - (1.0 - c * c) / (eta * eta)
    ci, ct = np.abs(c), np.sqrt(np.maximum(t2, 0.0))
    rs = (ci - eta * ct) / (ci + eta * ct)
    rp = (eta * ci - ct) / (eta * ci + ct)
    return np.where(t2 < 0.0, 1.0, (rs * rs + rp * rp) / 2.0)


def _smith_masking(v, n, roughness):  # pbr.rs:145-152
    alpha = roughness * roughness
    a2 = alpha * alpha
    z2 = _dot(v, n) ** 2
    lam = (-1.0 + np.sqrt(1.0 + a2 * (1.0 - z2) / z2)) / 2.0
    return 1.0 / (1.0 + lam)


def _to_local(n, tang0, v, rot):  # hitable.rs:37-41
    tang = np.cos(rot) * tang0 - np.sin(rot) * np.cross(n, tang0)
    bitang = np.cross(n, tang)
    return np.stack([_dot(v, tang), _dot(v, bitang), _dot(v, n)], axis=-1)


def attenuation(type, tex0, tex1, p0, p1, p2, n, on, rd, dir_o):
    """-> [m, 3] float64.  type: the material tag 6..12; tex0, tex1: the texture values at the hits, (3,) or [m, 3]; p0..p2: the
    material's parameters; n: the shading normals, on: the object-space outward normals (DisneyMetal's tangent, hitable.rs:96), rd: the
    incoming and dir_o the scattered directions, [m, 3] each."""
    n, on, rd, dir_o = (np.asarray(x, np.float64).reshape(-1, 3) for x in (n, on, rd, dir_o))
    m = len(n)
    tex0 = np.broadcast_to(np.asarray(tex0, np.float64), (m, 3))
    p0, p1, p2 = float(p0), float(p1), float(p2)
    with np.errstate(all="ignore"):
        n_dot_i, n_dot_o = _dot(n, -rd), _dot(n, dir_o)
        h = _unit(dir_o - rd)
        h_dot_i, h_dot_o, n_dot_h = _dot(h, -rd), _dot(h, dir_o), _dot(n, h)
        if type == 6:  # OrenNayar pbr.rs:17-42
            cos_i, cos_o = np.abs(_dot(n, rd)), n_dot_o
            sin_i, sin_o = np.sqrt(1.0 - cos_i * cos_i), np.sqrt(1.0 - cos_o * cos_o)
            max_cos = np.maximum(cos_i * cos_o + sin_i * sin_o, 0.0)
            r2 = p0 * p0
            a = 1.0 - _c(0.5) * r2 / (r2 + _c(0.33))
            b = _c(0.45) * r2 / (r2 + _c(0.09))
            first = cos_i > cos_o
            sin_alpha, tan_beta = np.where(first, sin_o, sin_i), np.where(first, sin_i / cos_i, sin_o / cos_o)
            w = a + b * max_cos * sin_alpha * tan_beta
            return tex0 * (w * 2.0 * cos_o)[:, None]
        if type == 7:  # BurleyDiffuse pbr.rs:50-69
            fd90 = 0.5 + 2.0 * h_dot_o * h_dot_o * p0
            fd = _lerp(1.0, fd90, _schlick(n_dot_o)) * _lerp(1.0, fd90, _schlick(n_dot_i))
            return tex0 * (fd * 2.0 * n_dot_o)[:, None]
        if type == 8:  # RoughPlastic pbr.rs:160-189: tex0 the specular colour, tex1 the diffuse one, p1 eta
            kd = np.broadcast_to(np.asarray(tex1, np.float64), (m, 3))
            roughness = min(max(p0, _c(0.01)), 1.0)
            f_o = _fresnel_dielectric_2(h_dot_o, p1)
            d = _gtr2(n_dot_h, roughness)
            g = _smith_masking(-rd, n, roughness) * _smith_masking(dir_o, n, roughness)
            spec = tex0 * (g * f_o * d / (4.0 * n_dot_i * n_dot_o))[:, None]
            f_i = _fresnel_dielectric_2(h_dot_i, p1)
            diff = kd * ((1.0 - f_o) * (1.0 - f_i) * FRAC_1_PI)[:, None]
            return (spec + diff) * (n_dot_o * 2.0 * PI)[:, None]
        if type == 9:  # DisneyDiffuse pbr.rs:198-222: p1 subsurface
            fo, fi = _schlick(n_dot_o), _schlick(n_dot_i)
            fd90 = 0.5 + 2.0 * h_dot_o * h_dot_o * p0
            fd = _lerp(1.0, fd90, fo) * _lerp(1.0, fd90, fi)
            fss90 = p0 * h_dot_o * h_dot_o
            fss = _c(1.25) * (_lerp(1.0, fss90, fi) * _lerp(1.0, fss90, fo) * (1.0 / (n_dot_i + n_dot_o) - 0.5) + 0.5)
            return tex0 * (_lerp(fd, fss, p1) * 2.0 * n_dot_o)[:, None]
        if type == 10:  # DisneyMetal pbr.rs:232-278: p1 anisotropic, p2 rot
            fm = tex0 + (1.0 - tex0) * _schlick(h_dot_o)[:, None]
            alpha_min = _c(0.0001)
            if p1 > -10.0:
                aspect = np.sqrt(1.0 - _c(0.9) * p1)
                ax, ay = max(p0 * p0 / aspect, alpha_min), max(p0 * p0 * aspect, alpha_min)
                rot = p2 * 2.0 * PI
                tang = _unit(np.cross(np.array([0.0, 1.0, 0.0]), on))  # hitable.rs:96: from the outward normal
                dm = _gtr2_aniso(_to_local(n, tang, h, rot), ax, ay)
                gm = _smith_ggx_aniso(_to_local(n, tang, -rd, rot), ax, ay) * _smith_ggx_aniso(_to_local(n, tang, dir_o, rot), ax, ay)
            else:
                r2 = max(p0 * p0, alpha_min)
                dm = _gtr2(n_dot_h, r2)
                gm = _smith_ggx(n_dot_i, r2) * _smith_ggx(n_dot_o, r2)
            return fm * (dm * gm * n_dot_o * 2.0 * PI)[:, None]
        if type == 11:  # DisneySheen pbr.rs:286-308: p0 tint
            lum = (tex0 * np.array([_c(0.3), _c(0.6), _c(0.1)])).sum(axis=-1)
            c_tint = np.where((lum > 0.0)[:, None], tex0 / lum[:, None], 1.0)
            c_sheen = 1.0 + (c_tint - 1.0) * p0
            return c_sheen * (_schlick(h_dot_o) * n_dot_o * 2.0 * PI)[:, None]
        if type == 12:  # DisneyClearcoat pbr.rs:314-335: p0 gloss
            fc = _lerp(_c(0.4), 1.0, _schlick(h_dot_o))
            dc = _gtr1(n_dot_h, _lerp(_c(0.1), _c(0.001), p0))
            gc = _smith_ggx(n_dot_i, 0.25) * _smith_ggx(n_dot_o, 0.25)
            return np.repeat((0.25 * fc * dc * gc * n_dot_o * 2.0 * PI)[:, None], 3, axis=1)
    raise ValueError("not a pbr.rs material: tag %r" % (type,))


def sensitivity(type, tex0, tex1, p0, p1, p2, n, on, rd, dir_o, seed=0):
    """-> S [m]: the largest relative change of a component of attenuation() over N_PROBES evaluations in which every component of n, rd
    and dir_o is moved by an amount uniform within +-1 binary32 ulp of it.  `on` moves with n: by the same amounts, mirrored where the
    ray met the surface from inside (n = -on; below a RotateY the object-space normal is a rotation of that, which the size of the
    move does not feel).  A component that is 0 and stays 0 has not changed; one that leaves 0 has changed without bound."""
    n, on, rd, dir_o = (np.asarray(x, np.float64).reshape(-1, 3) for x in (n, on, rd, dir_o))
    rng = np.random.default_rng(seed)
    base = attenuation(type, tex0, tex1, p0, p1, p2, n, on, rd, dir_o)
    side = np.where(_dot(n, on) < 0.0, -1.0, 1.0)[:, None]
    S = np.zeros(len(n))

    def moved(x):
        step = rng.uniform(-1.0, 1.0, x.shape) * np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
        return x + step, step
    with np.errstate(all="ignore"):
        for _ in range(N_PROBES):
            n1, dn = moved(n)
            a = attenuation(type, tex0, tex1, p0, p1, p2, n1, on + side * dn, moved(rd)[0], moved(dir_o)[0])
            rel = np.where(a == base, 0.0, np.abs(a - base) / np.abs(base))
            S = np.maximum(S, np.nan_to_num(rel, nan=np.inf).max(axis=1))
    return S
