"""A set-valued reference of the image lookups (Sphere::get_uv hitable.rs:65-71, ImageTex::value texture.rs:183-193, tex_sky_color
demo_scene.rs:22-26) and of the checker's colour (texture.rs:40-49), in numpy, without a GPU.

The f32 normal of a hit (or the direction of a sky lookup) is the same bits everywhere: + - * / and sqrt are IEEE on the device, in
the oracle and here.  What differs between correct implementations is the last bits of acos and atan2.  So the angles are taken in
float64, rounded to f32, and EVERY f32 value within E_ACOS / E_ATAN2 ulp of the float64 value is a candidate (clipped to [0, pi_f32]
and [-pi_f32, pi_f32], the ranges the functions are specified to return).  Each candidate goes through the exact f32 chain that
follows — + PI, / (2 PI), / PI, the sky's 1 - u, the clamp that keeps NaN, 1 - v, * W, * H, the saturating truncation that maps NaN to
0, min(.., W - 1) — and the texels (i, j) that come out are what a correct implementation may read: one texel for all but the rays
that sit on a texel border.  When |n.y| > 1 (a rounded normal at a pole, a direction a hair longer than 1) acos is NaN for every
implementation, and the lookup reads row 0: the TOP row at the SOUTH pole.

E_ACOS = 4 and E_ATAN2 = 6, E_SIN = 4 are the single-precision bounds of the OpenCL full profile, to which the device's math library is
specified; they are not taken from what any kernel returns (the measured maxima: DESIGN.md 4).

The vectorised Sphere::hit below is tests/golden/np_ref.py's, operation for operation (its helpers work on tuples of arrays as they do on
tuples of scalars; only its branches are written as selections); tests/test_uv_ref_host.py holds it against np_ref ray by ray."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import np_ref  # noqa: E402

f32 = np.float32
PI = f32(np.pi)
TWO_PI = f32(2.0) * PI
FLT_MAX = np.finfo(f32).max
E_ACOS, E_ATAN2, E_SIN = 4, 6, 4


# ---- hits: the f32 local outward normal --------------------------------------------------------------------------------------------
def _cols(a):
    a = np.asarray(a, dtype=f32)
    return (a[..., 0], a[..., 1], a[..., 2])


def sphere_hit(c, r, o, d, t_min=1e-3, t_max=FLT_MAX):
    """np_ref.sphere_hit for rays o, d [n, 3]; c [3] or [n, 3] (a centre per ray: a moving sphere).  -> dict(hit [n] bool, t [n], p, on [n, 3])."""
    c, o, d, r = _cols(c), _cols(o), _cols(d), f32(r)
    t_min, t_max = f32(t_min), f32(t_max)
    with np.errstate(all="ignore"):
        oc = np_ref.sub(o, c)
        a = np_ref.dot(d, d)
        half_b = np_ref.dot(oc, d)
        cc = np_ref.dot(oc, oc) - r * r
        disc = half_b * half_b - a * cc
        sqrtd = np.sqrt(disc)
        r1 = (-half_b - sqrtd) / a
        r2 = (-half_b + sqrtd) / a
        bad1 = (r1 < t_min) | (t_max < r1)
        bad2 = (r2 < t_min) | (t_max < r2)
        root = np.where(bad1, r2, r1).astype(f32)
        hit = ~(disc < f32(0.0)) & ~(bad1 & bad2) & ~np.isnan(disc)
        p = np_ref.add(o, np_ref.scale(d, root))
        on = np_ref.divs(np_ref.sub(p, c), r)
    return {"hit": hit, "t": root, "p": np.stack(p, axis=-1).astype(f32), "on": np.stack(on, axis=-1).astype(f32)}


def rotate_y_ray(sin_t, cos_t, o, d):
    """the ray RotateY::hit hands to its object (np_ref.rotate_y_sphere_hit's `ro`, `rd`)"""
    sin_t, cos_t = f32(sin_t), f32(cos_t)
    o, d = _cols(o), _cols(d)
    ro = (cos_t * o[0] - sin_t * o[2], o[1], sin_t * o[0] + cos_t * o[2])
    rd = (cos_t * d[0] - sin_t * d[2], d[1], sin_t * d[0] + cos_t * d[2])
    return np.stack(ro, axis=-1).astype(f32), np.stack(rd, axis=-1).astype(f32)


def translate_ray(offset, o):
    """the origin Translate::hit hands to its object (np_ref.translate_hit)"""
    return np.stack(np_ref.sub(_cols(o), _cols(offset)), axis=-1).astype(f32)


# ---- candidates -----------------------------------------------------------------------------------------------------------------------
def _ordered(x):
    """f32 -> int64 that orders like the reals (both zeros -> 0)"""
    b = np.asarray(x, dtype=f32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _from_ordered(k):
    k = np.asarray(k, dtype=np.int64)
    return np.where(k < 0, (-k) | 0x80000000, k).astype(np.uint32).view(f32)


def within_ulp(ref64, e, lo, hi):
    """Every f32 within e ulp of the float64 values ref64 [n], clipped to [lo, hi]: float32 [n, 4 e + 1], a row's values repeated where fewer
    qualify.  One ulp is the f32 spacing at the reference (2^(exponent - 23)); floats below a power of two lie half as far apart, hence
    2 e steps either way, each kept by its distance.  A NaN reference gives a row of NaN."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    nan = np.isnan(ref64)
    safe = np.where(nan, 0.0, ref64)
    mid = safe.astype(f32)
    ulp = 2.0 ** (np.maximum(np.frexp(np.abs(safe))[1], -125) - 24)
    steps = np.arange(-2 * e, 2 * e + 1, dtype=np.int64)
    cand = _from_ordered(_ordered(mid)[:, None] + steps[None, :])
    keep = np.abs(cand.astype(np.float64) - safe[:, None]) <= e * ulp[:, None]
    keep[:, 2 * e] = True  # (the correctly rounded value)
    cand = np.where(keep, cand, mid[:, None])
    cand = np.clip(cand, f32(lo), f32(hi)).astype(f32)
    cand[nan] = np.nan
    return cand


def clamp01(x):
    """Rust's f32::clamp(0, 1): NaN stays NaN"""
    x = np.asarray(x, dtype=f32)
    return np.where(x < f32(0.0), f32(0.0), np.where(x > f32(1.0), f32(1.0), x)).astype(f32)


def as_u32(x):
    """Rust's `x as u32`: toward zero, saturating, NaN -> 0 (as int64)"""
    x = np.asarray(x, dtype=f32).astype(np.float64)
    return np.clip(np.trunc(np.where(np.isnan(x), 0.0, x)), 0.0, 4294967295.0).astype(np.int64)


def texel_index(u, v, w, h):
    """ImageTex::value's (i, j) for f32 u, v (texture.rs:183-193)"""
    with np.errstate(all="ignore"):
        uu = clamp01(u)
        vv = (f32(1.0) - clamp01(v)).astype(f32)
        i = np.minimum(as_u32((uu * f32(w)).astype(f32)), w - 1)
        j = np.minimum(as_u32((vv * f32(h)).astype(f32)), h - 1)
    return i, j


def candidates(n, w, h, sky=False, e_acos=E_ACOS, e_atan2=E_ATAN2):
    """The texels a correct implementation may read for the f32 normals (sky: directions) n [m, 3] of a w x h image.
    -> dict(I [m, 4 e_atan2 + 1], J [m, 4 e_acos + 1]: the candidate columns and rows (the set is their product), single [m] bool,
    nan_row [m] bool: |n.y| > 1, v is NaN for every candidate, i0, j0 [m]: the texel of the correctly rounded angles)."""
    n = np.asarray(n, dtype=f32)
    with np.errstate(all="ignore"):
        theta = within_ulp(np.arccos(-n[:, 1].astype(np.float64)), e_acos, 0.0, PI)
        phi = within_ulp(np.arctan2(-n[:, 2].astype(np.float64), n[:, 0].astype(np.float64)), e_atan2, -PI, PI)
        u = ((phi + PI).astype(f32) / TWO_PI).astype(f32)
        v = (theta / PI).astype(f32)
        if sky:
            u = (f32(1.0) - u).astype(f32)
    I, J = texel_index(u, v[:, :1], w, h)[0], texel_index(u[:, :1], v, w, h)[1]
    nan_row = np.abs(n[:, 1]) > f32(1.0)
    assert np.array_equal(nan_row, np.isnan(theta).all(axis=1)) and not J[nan_row].any()
    single = (I.min(axis=1) == I.max(axis=1)) & (J.min(axis=1) == J.max(axis=1))
    return {"I": I, "J": J, "single": single, "nan_row": nan_row, "i0": I[:, 2 * e_atan2], "j0": J[:, 2 * e_acos]}


def in_set(cand, i, j):
    """[m] bool: texel (i, j) is one of the ray's candidates"""
    return (cand["I"] == np.asarray(i)[:, None]).any(axis=1) & (cand["J"] == np.asarray(j)[:, None]).any(axis=1)


# ---- test images: a texel's colour names the texel ----------------------------------------------------------------------------------
def make_image(w, h, eight_bit, decoy=False):
    """float pool: texel (i, j) = (i + 0.5, j + 0.5, 0.25); 8-bit pool (w, h <= 256): (i / 255, j / 255, ((7 i + 13 j) % 256) / 255).
    A decoy differs from every image under test in its third component (0.75; (7 i + 13 j + 101) % 256)."""
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if eight_bit:
        assert w <= 256 and h <= 256
        k = np.stack([i, j, (7 * i + 13 * j + (101 if decoy else 0)) % 256], axis=-1)
        return (k.astype(f32) / f32(255.0)).astype(f32)
    return np.stack([i + 0.5, j + 0.5, np.full_like(i, 0.75 if decoy else 0.25, dtype=np.float64)], axis=-1).astype(f32)


def decode(colour, w, h, eight_bit, squared=False):
    """The texel (i, j) whose colour `colour` [m, 3] is, bit for bit (squared: the f32 square the sky returns); (-1, -1) where it is the
    colour of no texel of the image."""
    img = make_image(w, h, eight_bit)
    if squared:
        img = (img * img).astype(f32)
    colour = np.ascontiguousarray(colour, dtype=f32)
    r, g = img[0, :, 0], img[:, 0, 1]
    assert np.all(np.diff(r.astype(np.float64)) > 0) and np.all(np.diff(g.astype(np.float64)) > 0)
    with np.errstate(all="ignore"):
        i = np.clip(np.searchsorted(r, colour[:, 0]), 0, w - 1)
        j = np.clip(np.searchsorted(g, colour[:, 1]), 0, h - 1)
    ok = (img[j, i].view(np.uint32) == colour.view(np.uint32)).all(axis=1)
    return np.where(ok, i, -1), np.where(ok, j, -1)


# ---- ray groups -------------------------------------------------------------------------------------------------------------------------
GROUPS = ("random", "pole_north", "pole_south", "seam", "border", "axes")
N_GROUP = 20000


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def normalize_f32(d):
    """glam's normalize in f32: v * (1 / length), dot = (xx + yy) + zz"""
    d = np.asarray(d, dtype=f32)
    ln = np.sqrt(np_ref.dot(_cols(d), _cols(d))).astype(f32)
    return (d * (f32(1.0) / ln)[:, None]).astype(f32)


def group_rays(group, c, r, w, h, seed=0, n=N_GROUP, to_world=None):
    """Rays of one group at the sphere (c, r), origins at 4 |r| on the visible side, aimed at targets given in the sphere's LOCAL frame
    (to_world: maps local points [m, 3] float64 to world; None: the identity).  -> o, d float32 [n, 3], d normalised in f32.
      random      targets uniform on the sphere
      pole_north / pole_south   c +- r e_y plus 1e-3 r of xz noise
      seam        local x < 0, |z| <= 1e-7 r: where atan2 jumps from -pi to pi
      border      phi = 2 pi k / w - pi, theta = pi m / h: the texel borders
      axes        the six axis normals, head-on, from origins that are representable"""
    rng = np.random.default_rng([seed, GROUPS.index(group)])
    c, ra = np.asarray(c, dtype=np.float64), abs(float(r))
    if group == "axes":
        assert to_world is None
        e = np.concatenate([np.eye(3), -np.eye(3)])
        o = (c.astype(f32)[None, :] + (f32(4.0 * ra) * e).astype(f32)).astype(f32)  # (one coordinate moves: the other two stay the centre's)
        return o, (-e).astype(f32)
    if group == "random":
        nrm = _unit(rng.normal(size=(n, 3)))
    elif group in ("pole_north", "pole_south"):
        nrm = np.zeros((n, 3))
        nrm[:, 1] = 1.0 if group == "pole_north" else -1.0
        nrm[:, [0, 2]] = rng.uniform(-1e-3, 1e-3, (n, 2))
    elif group == "seam":
        th = rng.uniform(0.05, np.pi - 0.05, n)
        nrm = np.stack([-np.sin(th), np.cos(th), rng.uniform(-1e-7, 1e-7, n)], axis=1)
        nrm[: n // 8, 2] = 0.0
    elif group == "border":
        k, m = rng.integers(0, w + 1, n), rng.integers(0, h + 1, n)
        on_u = rng.random(n) < 0.5  # a ray sits on a column border or on a row border, at a random place along it
        phi = np.where(on_u, 2.0 * np.pi * k / w - np.pi, rng.uniform(-np.pi, np.pi, n))
        th = np.where(on_u, rng.uniform(0.02, np.pi - 0.02, n), np.pi * m / h)
        # get_uv: theta = acos(-y), phi = atan2(-z, x)
        nrm = np.stack([np.sin(th) * np.cos(phi), -np.cos(th), -np.sin(th) * np.sin(phi)], axis=1)
    else:
        raise ValueError(group)
    tgt = c + float(r) * nrm  # (p - c) / r = nrm: with a negative radius the normal of the lookup points inwards
    geo = _unit(nrm) * np.sign(float(r))
    view = _unit(geo + 0.35 * rng.normal(size=(n, 3)))  # the visible side of the target
    view = np.where((np.sum(view * geo, axis=1) > 0.3)[:, None], view, geo)
    org = c + 4.0 * ra * view
    if to_world is not None:
        tgt, org = to_world(tgt), to_world(org)
    o = org.astype(f32)
    return o, normalize_f32((tgt - o.astype(np.float64)).astype(f32))


def sky_directions(seed=0, n=N_GROUP):
    """-> dict(name: directions float32 [m, 3]): random unit vectors, cones of 1e-4 around +-y, and the forced ones — (0, +-nextafter(1, 2), 0)
    (|d|^2 = 1.0000002 passes the near-one window of main.rs:39 and acos is NaN), (0, +-nextafter(1, 0), 0), the seam (-1, 0, +-0), (0, 0, +-1)."""
    rng = np.random.default_rng([seed, 77])
    up, dn = np.nextafter(f32(1), f32(2)), np.nextafter(f32(1), f32(0))
    out = {"random": normalize_f32(rng.normal(size=(n, 3)).astype(f32))}
    for name, s in (("cone_up", 1.0), ("cone_down", -1.0)):
        v = np.stack([rng.uniform(-1e-4, 1e-4, n), np.full(n, s), rng.uniform(-1e-4, 1e-4, n)], axis=1)
        out[name] = normalize_f32(v.astype(f32))
    out["forced"] = np.array([[0, up, 0], [0, -up, 0], [0, dn, 0], [0, -dn, 0], [-1, 0, 0.0], [-1, 0, -0.0], [0, 0, 1], [0, 0, -1]], dtype=f32)
    return out


def check_group(group, cand, hit, w, h):
    """The conditions that keep a group from passing emptily, on the reference's side alone (tests/test_uv_ref_host.py prints what they read).
    -> dict(hits, ambiguous, nan_row: shares of the hits)."""
    k = hit.astype(bool)
    nh = int(k.sum())
    st = {"hits": nh, "ambiguous": float((~cand["single"][k]).mean()), "nan_row": float(cand["nan_row"][k].mean())}
    assert nh >= (6 if group == "axes" else 0.9 * len(hit)), (group, st)
    i0, j0 = cand["i0"][k], cand["j0"][k]
    if group == "border":  # (a 1 x 1 or 1 x 3 image has no borders in one direction or in both: its rays are a second random group)
        assert st["ambiguous"] >= 0.20 or w == 1 or h == 1, (group, st)
    elif group != "axes":
        assert st["ambiguous"] <= 0.005, (group, w, h, st)
    return st, i0, j0


# ---- checker --------------------------------------------------------------------------------------------------------------------------
def checker(p, e=E_SIN):
    """CheckerTex::value at the f32 points p [m, 3]: sin(10 x) sin(10 y) sin(10 z) < 0 picks the first ("odd") colour.  The sines are
    taken in float64 of the f32 arguments fl(10 p).  -> (negative [m] bool, decided [m] bool): a ray is decided when no factor is within
    e ulp of changing sign; a factor of exactly +-0 makes the product +-0, which is not negative whatever the others are."""
    p = np.asarray(p, dtype=f32)
    arg = (p * f32(10.0)).astype(f32)
    s = np.sin(arg.astype(np.float64))
    zero = (arg == 0).any(axis=1)
    # a result within e ulp of zero could come out with either sign, or as a zero; |sin| of a nonzero f32 is never that small unless the argument is
    tiny = np.abs(s) <= e * 2.0 ** -149
    underflow = np.abs(s[:, 0] * s[:, 1] * s[:, 2]) < 2.0 ** -120  # (the f32 product may round to a zero: tiny arguments only)
    decided = zero | ~(tiny.any(axis=1) | underflow)
    negative = ~zero & ((s < 0).sum(axis=1) % 2 == 1)
    return negative, decided
