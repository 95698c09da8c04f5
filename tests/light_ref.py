"""Light importance sampling (rt_set_lights, DESIGN.md "Light sampling") in numpy float32, every operation rounded once in the kernels'
order: the set-up of a light, the selection between the material's own direction and a light, the light draw, p_L, the weight and the
weighted attenuation.  The oracle knows no light sampling, so this restatement is the reference of tests/test_lights.py,
tests/test_lights_materials.py and tests/test_lights_host.py.  Hit records come from tests/golden/np_ref.py and tests/quad_ref.py; the quad
test inside p_L is quad_ref.hit_one; the family's BRDF at the chosen direction is np_ref.family_attenuation, the one statement np_ref.scatter
uses too (`tex`, `tex1` and p0..p2 of `mat` pass through); unaffected materials go through np_ref.scatter unchanged."""
import numpy as np

import quad_ref

np_ref = quad_ref.np_ref
f32 = np.float32
FLT_MAX = np.finfo(f32).max
FAMILY = (2, 6, 7, 8, 9, 10, 11, 12)  # Lambert and the seven pbr.rs materials: random_on_hemisphere, p_s = 0.5 / pi
AFFECTED = (1,) + FAMILY


def setup(q, u, v):
    """(normal, D, w) as quad_ref.setup and area = sqrt(dot(n, n)), n = cross(u, v), per light"""
    q, u, v = (np.asarray(x, dtype=f32).reshape(-1, 3) for x in (q, u, v))
    normal, D, w = quad_ref.setup(q, u, v)
    n = quad_ref.cross(u, v)
    area = np.sqrt(quad_ref.dot(n, n).astype(f32)).astype(f32)
    return {"n": len(q), "q": q, "u": u, "v": v, "normal": normal, "D": D, "w": w, "area": area}


def p_light(L, po, d):
    """p_L of the rays (po, d) [m, 3] float32: (sum_k pdf_k) / n in index order, pdf_k = t t / (|dot(normal_k, d)| area_k) where the quad
    test accepts the ray with t_min = 1e-3, t_max = FLT_MAX.  Returns (p_L [m] float32, how many lights contributed [m])."""
    po, d = np.asarray(po, dtype=f32).reshape(-1, 3), np.asarray(d, dtype=f32).reshape(-1, 3)
    total = np.zeros(len(po), f32)
    count = np.zeros(len(po), np.int64)
    with np.errstate(all="ignore"):
        for k in range(L["n"]):
            ok, t, _, _ = quad_ref.hit_one(L["q"][k], L["u"][k], L["v"][k], quad_ref.QUAD, L["normal"][k], L["D"][k], L["w"][k], po, d,
                                           1e-3, FLT_MAX)
            den = (np.abs(quad_ref.dot(np.broadcast_to(L["normal"][k], d.shape), d).astype(f32)) * L["area"][k]).astype(f32)
            pdf = ((t * t).astype(f32) / den).astype(f32)
            total = np.where(ok, (total + pdf).astype(f32), total)
            count += ok
        return (total / f32(L["n"])).astype(f32), count


def light_dir(L, rng, po):
    """k = min((uint32)(next() n), n - 1); a = next(); b = next(); target = (Q_k + u_k a) + v_k b; normalize(target - po)"""
    k = min(int(rng.next() * f32(L["n"])), L["n"] - 1)
    a = rng.next()
    b = rng.next()
    Q, u, v = (tuple(f32(x) for x in L[key][k]) for key in ("q", "u", "v"))
    target = np_ref.add(np_ref.add(Q, np_ref.scale(u, a)), np_ref.scale(v, b))
    with np.errstate(all="ignore"):
        return np_ref.normalize(np_ref.sub(target, po)), k


def scatter(mat, rd, rec, rng, L):
    """One hit with the light set L (None or n 0: np_ref.scatter).  Returns (alive, attenuation, o, d, emitted, info); info names the
    branch ("own", "light" or None for an unaffected material), c, p_L, how many lights contributed, the weight and (of a live ray) the
    attenuation before the weight."""
    ty = mat["type"]
    if L is None or L["n"] == 0 or ty not in AFFECTED:
        return np_ref.scatter(mat, rd, rec, rng) + ({"branch": None},)
    n, p = rec["n"], rec["p"]
    tex = tuple(f32(x) for x in mat.get("tex", (0, 0, 0)))
    po = np_ref.offset_hit_point(p, n)
    s = rng.next()
    if s < f32(0.5):
        branch = "own"
        if ty == 1:
            sd = np_ref.add(n, np_ref.normalize(np_ref.random_in_unit_sphere(rng)))
            eps = f32(np.finfo(np.float32).eps)
            if abs(sd[0]) < eps and abs(sd[1]) < eps and abs(sd[2]) < eps:
                sd = n
            d = np_ref.normalize(sd)
        else:
            d = np_ref.random_on_hemisphere(rng, n)
    else:
        branch = "light"
        d, _ = light_dir(L, rng, po)
    c = np_ref.dot(n, d)
    info = {"branch": branch, "c": c, "p_L": f32(0), "n_contrib": 0, "wgt": f32(0)}
    if not (c > f32(0.0)):
        return False, np_ref.v3(1, 1, 1), po, d, np_ref.ZERO, info
    pl, cnt = p_light(L, np.array([po], f32), np.array([d], f32))
    p_l = f32(pl[0])
    p_s = c * np_ref.FRAC_1_PI if ty == 1 else f32(0.5) * np_ref.FRAC_1_PI
    wgt = p_s / ((p_s + p_l) * f32(0.5))
    att = tex if ty == 1 else np_ref.family_attenuation(mat, rd, rec, d)
    info.update(p_L=p_l, n_contrib=int(cnt[0]), wgt=wgt, att=att)
    return True, np_ref.scale(att, wgt), po, d, np_ref.ZERO, info
