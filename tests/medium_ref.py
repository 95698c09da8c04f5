"""The set of admissible outcomes of ONE ray in a world that holds ConstantMedium entries (hitable.rs:523-588).

ConstantMedium::hit is the one closest-hit routine whose result goes through a libm-class function: hit_dist = neg_inv_density * ln(xi).
Everything else in it is IEEE binary32 arithmetic, and this module restates that part exactly, operation for operation, vectorised over
rays in numpy float32 (glam order: dot = (xx + yy) + zz), from the flat arrays of scene.arrays():

  * the ray the medium receives: the world ray through the wrappers AROUND the medium (med_xform and its parents, outermost first);
  * boundary.hit(r, -inf, inf) and boundary.hit(r, t1 + 0.0001, inf) over the boundary's primitives in list order, each below the rest
    of its own chain, with HitableList::hit's shrinking t_max (Sphere::hit hitable.rs:75-91, XYRect::hit 251-270, Translate 409-418,
    RotateY 482-510);
  * the clamps to t_min and t_max, `t1 >= t2`, `t1 < 0`; ray_len = |d| of the ray the medium receives; dist_inside, hit_dist, t and
    p = r.at(t), the point moved back out through the wrappers around the medium;
  * the draw xi: counter slot 224 + m of the depth block, or the block above 2^30 for the media from the 32nd on.

The logarithm is the only free part: L ranges over every binary32 value within LOG_ULP = 3 ulp of float64 log(xi) — the bound
test_libm_class_functions_are_within_their_ulp_bounds holds the device's logf to — and is exactly -inf for xi = 0.

For each choice of L, for every medium on the ray independently, and for each ACCEPTANCE RULE the world search has one outcome (hit index,
t, and p where a medium wins).  The rules:

  clamp   the media in entry order after the solid primitives, each with t_max = the closest hit so far, accepted whenever its hit()
          accepts: HitableList::hit (hitable.rs:117-132), the oracle's list walk and closest_hit_rects of the device.
  winner  every medium with t_max = FLT_MAX, then the smallest t, a tie to the later entry: leaf_test / media_step of the tree.

`outcomes` enumerates the product of the per-medium choices as a set of states (closest t so far, hit index) that is carried from one
medium to the next and stripped of duplicates after each: an exact enumeration, since a medium's result depends on the earlier media only
through that state.  The set is the reference.  The closest SOLID hit has no free part; it is taken from the oracle's list walk over
the same scene built without its media (tests/medium_edge_cases.py builds both) and enters as the first state.

One deviation of the kernels from hitable.rs is part of the contract (rect_root, rt_device.h): a NaN plane distance — an origin in a
rectangle's plane with a direction inside it, 0/0 — is rejected, where the reference's comparisons all fail on it and report a hit at
t = NaN.  `nan_plane` selects the convention: "reference" for the oracle, "rejected" for the device."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import np_ref  # noqa: E402
from helpers import ctr_draw  # noqa: E402

f32 = np.float32
NONE = 0xFFFFFFFF
FLT_MAX = np.finfo(f32).max
T_MIN = f32(1e-3)
LOG_ULP = 3.0
N_L = 7  # candidates around the rounded float64 logarithm, -3 .. +3 binary32 steps
INF = f32(np.inf)


def bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cols(v):
    v = np.asarray(v, dtype=f32)
    return (v[..., 0], v[..., 1], v[..., 2])


# ---- wrappers ---------------------------------------------------------------------------------------------------------------------
def _chain(a, x, stop=NONE):
    """the wrappers from x outwards up to (not including) `stop`"""
    out = []
    x, stop = int(x), int(stop)
    while x != stop and x != NONE:
        out.append(x)
        x = int(a["xf_parent"][x])
    return out


def _xform_ray(a, x, o, d):
    q = a["xf_param"][4 * x:4 * x + 4].astype(f32)
    if int(a["xf_type"][x]) == 0:  # Translate hitable.rs:411
        return (o[0] - q[0], o[1] - q[1], o[2] - q[2]), d
    s, c = q[0], q[1]             # RotateY hitable.rs:483-492
    return (c * o[0] - s * o[2], o[1], s * o[0] + c * o[2]), (c * d[0] - s * d[2], d[1], s * d[0] + c * d[2])


def _xform_point_back(a, x, p):
    q = a["xf_param"][4 * x:4 * x + 4].astype(f32)
    if int(a["xf_type"][x]) == 0:  # hitable.rs:413
        return (p[0] + q[0], p[1] + q[1], p[2] + q[2])
    s, c = q[0], q[1]             # hitable.rs:495-498
    return (c * p[0] + s * p[2], p[1], -s * p[0] + c * p[2])


def to_object(a, x, stop, o, d):
    for w in reversed(_chain(a, x, stop)):  # the outermost wrapper moves the ray first
        o, d = _xform_ray(a, w, o, d)
    return o, d


# ---- primitives -------------------------------------------------------------------------------------------------------------------
def _sphere_t(c, r, o, d, t_min, t_max):
    oc = (o[0] - c[0], o[1] - c[1], o[2] - c[2])
    aa = _dot(d, d)
    half_b = _dot(oc, d)
    cc = _dot(oc, oc) - r * r
    disc = half_b * half_b - aa * cc
    sq = np.sqrt(disc)
    r0 = (-half_b - sq) / aa
    r1 = (-half_b + sq) / aa
    bad0 = (r0 < t_min) | (t_max < r0)
    bad1 = (r1 < t_min) | (t_max < r1)
    return ~(disc < f32(0.0)) & ~(bad0 & bad1), np.where(bad0, r1, r0), disc


def _rect_t(axis, mn, mx, o, d, t_min, t_max, reject_nan):
    t = (mn[axis] - o[axis]) / d[axis]
    bad = (t < t_min) | (t > t_max)
    if reject_nan:
        bad = bad | (t != t)
    p = tuple(o[k] + d[k] * t for k in range(3))
    ua, va = ((1, 2), (0, 2), (0, 1))[axis]
    out = (p[ua] < mn[ua]) | (p[ua] > mx[ua]) | (p[va] < mn[va]) | (p[va] > mx[va])
    return ~bad & ~out, t


class World:
    """the flat arrays of a scene, and what of them the medium search needs"""

    def __init__(self, scene):
        self.a = a = scene.arrays()
        self.ns, self.nr, self.n_media = int(scene.flat.n_spheres), int(scene.flat.n_rects), int(scene.flat.n_media)
        self.n_prims = self.ns + self.nr
        med = np.concatenate([a["sph_medium"] if len(a["sph_medium"]) else np.full(self.ns, NONE, np.uint32),
                              a["rect_medium"] if len(a["rect_medium"]) else np.full(self.nr, NONE, np.uint32)]).astype(np.int64)
        self.prim_medium = med
        self.solid_ids = np.nonzero(med == NONE)[0]  # index k of the scene built without its media is primitive solid_ids[k] here
        self.boundary = [np.nonzero(med == m)[0] for m in range(self.n_media)]
        self.med_xform = [int(a["med_xform"][m]) if len(a["med_xform"]) else NONE for m in range(self.n_media)]
        self.neg_inv_density = a["med_neg_inv_density"].astype(f32)  # (the host mirror folds the BvhNode multiplicity of hitable.rs:188 in)

    def prim_xform(self, i):
        a = self.a
        if i < self.ns:
            return int(a["sph_xform"][i]) if len(a["sph_xform"]) else NONE
        return int(a["rect_xform"][i - self.ns]) if len(a["rect_xform"]) else NONE

    def prim_t(self, i, o, d, t_min, t_max, reject_nan):
        a = self.a
        if i < self.ns:
            ok, t, _ = _sphere_t((a["sph_cx"][i], a["sph_cy"][i], a["sph_cz"][i]), a["sph_r"][i], o, d, t_min, t_max)
            return ok, t
        k = i - self.ns
        return _rect_t(int(a["rect_axis"][k]), a["rect_min"][3 * k:3 * k + 3], a["rect_max"][3 * k:3 * k + 3], o, d, t_min, t_max, reject_nan)

    def boundary_hit(self, m, ro, rd, t_min, t_max, reject_nan, cache):
        """boundary.hit(r, t_min, t_max) for the ray (ro, rd) the medium received -> (hit anything, t of the closest)"""
        closest = np.broadcast_to(f32(t_max), ro[0].shape).astype(f32)
        any_ = np.zeros(ro[0].shape, bool)
        for i in self.boundary[m]:
            x = self.prim_xform(int(i))
            if x not in cache:
                cache[x] = to_object(self.a, x, self.med_xform[m], ro, rd)
            po, pd = cache[x]
            ok, t = self.prim_t(int(i), po, pd, t_min, closest, reject_nan)
            closest = np.where(ok, t, closest).astype(f32)
            any_ |= ok
        return any_, closest

    def interval(self, m, o, d, nan_plane="rejected"):
        """The two boundary searches of medium m for the world rays (o, d) [n, 3] -> dict(ro, rd: the ray the medium receives; ok: both
        searches found a root; t1, t2: the roots, before any clamp; t_min2: the second search's t_min)"""
        reject = {"rejected": True, "reference": False}[nan_plane]
        with np.errstate(all="ignore"):
            ro, rd = to_object(self.a, self.med_xform[m], NONE, _cols(o), _cols(d))
            cache = {}
            ok1, t1 = self.boundary_hit(m, ro, rd, -INF, INF, reject, cache)
            t_min2 = (t1 + f32(0.0001)).astype(f32)
            ok2, t2 = self.boundary_hit(m, ro, rd, t_min2, INF, reject, cache)
        return dict(ro=ro, rd=rd, ok=ok1 & ok2, ok1=ok1, t1=t1, t2=t2, t_min2=t_min2)

    def point_out(self, m, p):
        """rec.p of medium m, given in the space of the ray it received, after the wrappers around it fixed the record"""
        for w in _chain(self.a, self.med_xform[m]):
            p = _xform_point_back(self.a, w, p)
        return p

    def albedo(self, m):
        """the constant colour of medium m's phase texture (None when the texture is not constant) and the texture's index"""
        a = self.a
        tex = int(a["mat_tex0"][int(a["med_mat"][m])])
        return (a["tex_color0"][3 * tex:3 * tex + 3].astype(f32) if int(a["tex_type"][tex]) == 0 else None), tex


# ---- the draw and the logarithm -----------------------------------------------------------------------------------------------------
def medium_counter(depth, m):
    base = (depth + 1) * 256
    return base + 224 + m if m < 32 else 0x40000000 + (base << 8) + m


def medium_xi(keys, depth, m):
    keys = np.asarray(keys, dtype=np.uint32)
    r = ctr_draw(keys[:, 0], keys[:, 1], np.full(len(keys), medium_counter(depth, m), np.uint64))
    return ((r >> 8).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)


def log_candidates(xi):
    """-> (L [n, N_L] binary32, valid [n, N_L]): every binary32 within LOG_ULP ulp of float64 log(xi) (the ulp taken at the reference, as
    test_libm_class_functions_are_within_their_ulp_bounds takes it); for xi = 0 the exact -inf alone.  Column N_L // 2 is the rounded
    float64 value, the `central` L."""
    with np.errstate(all="ignore"):
        ref = np.log(xi.astype(np.float64))
        c = ref.astype(f32)
        steps = np.arange(N_L, dtype=np.int64) - N_L // 2
        L = (c.view(np.uint32).astype(np.int64)[:, None] + steps[None, :]).astype(np.uint32).view(f32)
        ulp = 2.0 ** (np.maximum(np.frexp(np.abs(ref))[1], -125) - 24)
        valid = np.abs(L.astype(np.float64) - ref[:, None]) <= LOG_ULP * ulp[:, None]
    zero = xi == 0
    L[zero] = -INF
    valid[zero] = steps[None, :] == 0
    assert valid[:, N_L // 2].all()
    return L, valid


def isotropic_direction(keys, depth):
    """Isotropic::scatter's direction (material.rs:103-113): normalize(random_in_unit_sphere), the first draws of the depth block"""
    keys = np.asarray(keys, dtype=np.uint32)
    n = len(keys)
    out = np.zeros((n, 3), f32)
    todo = np.arange(n)
    ctr = (depth + 1) * 256
    two, m1 = f32(1.0) - f32(-1.0), f32(-1.0)
    while len(todo):
        v = []
        for k in range(3):
            r = ctr_draw(keys[todo, 0], keys[todo, 1], np.full(len(todo), ctr + k, np.uint64))
            v.append(((r >> 8).astype(f32) * f32(1.0 / 16777216.0)).astype(f32) * two + m1)
        ctr += 3
        acc = _dot(v, v) < f32(1.0)
        inv = f32(1.0) / np.sqrt(_dot(v, v)[acc])
        out[todo[acc]] = np.stack([v[0][acc] * inv, v[1][acc] * inv, v[2][acc] * inv], axis=1)
        todo = todo[~acc]
    return out


# ---- one medium, every L -------------------------------------------------------------------------------------------------------------
def medium_t(G, nid, L, t_max):
    """ConstantMedium::hit after the searches (hitable.rs:553-572), t_min = 0.001.  G: World.interval's result ([n]); L and t_max broadcast
    against [n, 1, ...] -> (accepted, t)"""
    ex = (slice(None),) + (None,) * (np.ndim(L) - 1)
    with np.errstate(all="ignore"):
        t1, t2 = G["t1"][ex], G["t2"][ex]
        t1 = np.where(t1 < T_MIN, T_MIN, t1)
        t2 = np.where(t2 > t_max, t_max, t2).astype(f32)
        ok = G["ok"][ex] & ~(t1 >= t2)
        t1 = np.where(t1 < f32(0.0), f32(0.0), t1)
        ray_len = np.sqrt(_dot(G["rd"], G["rd"]))[ex]
        dist_inside = (t2 - t1) * ray_len
        hit_dist = nid * L
        ok = ok & ~(hit_dist > dist_inside)
        t = (t1 + hit_dist / ray_len).astype(f32)
    return ok, t


def medium_t_set(W, m, o, d, keys, depth, t_max=FLT_MAX, nan_plane="rejected"):
    """every t medium m alone may report for the rays, one column per L (NaN where it does not accept or L is out of range): what a
    device `t` of a hit on medium m is held to where the rest of the world is not restated"""
    G = W.interval(m, o, d, nan_plane)
    L, valid = log_candidates(medium_xi(keys, depth, m))
    ok, t = medium_t(G, W.neg_inv_density[m], L, f32(t_max))
    return np.where(ok & valid, t, f32(np.nan)).astype(f32)


# ---- the world search ---------------------------------------------------------------------------------------------------------------
def _strip(tb, hit, valid):
    """drop duplicate states of every ray and close the columns up"""
    key = (hit.astype(np.int64) + 1) << 32 | tb.view(np.uint32).astype(np.int64)
    key = np.where(valid, key, np.int64(2 ** 62))
    order = np.argsort(key, axis=1, kind="stable")
    key, tb, hit, valid = (np.take_along_axis(x, order, axis=1) for x in (key, tb, hit, valid))
    valid[:, 1:] &= key[:, 1:] != key[:, :-1]
    order = np.argsort(~valid, axis=1, kind="stable")
    tb, hit, valid = (np.take_along_axis(x, order, axis=1) for x in (tb, hit, valid))
    keep = max(1, int(valid.sum(axis=1).max()))
    return tb[:, :keep].copy(), hit[:, :keep].copy(), valid[:, :keep].copy()


def outcomes(W, o, d, keys, depth, solid_hit, solid_t, rule, nan_plane="rejected", intervals=None):
    """The set of outcomes of the world search under `rule` ("clamp" or "winner") -> dict(hit [n, S] (-1 a miss), t [n, S], valid [n, S],
    p [n, S, 3] (of a medium's hit), n_hits [n]: distinct hit indices in the set).  solid_hit / solid_t: the closest solid primitive
    (index in THIS scene, -1 none)."""
    n = len(o)
    tb = np.where(solid_hit >= 0, solid_t, FLT_MAX).astype(f32)[:, None]
    hit = solid_hit.astype(np.int64)[:, None]
    valid = np.ones((n, 1), bool)
    Gs = []
    for m in range(W.n_media):
        G = intervals[m] if intervals is not None else W.interval(m, o, d, nan_plane)
        Gs.append(G)
        L, lv = log_candidates(medium_xi(keys, depth, m))
        if rule == "clamp":
            ok, t = medium_t(G, W.neg_inv_density[m], L[:, None, :], tb[:, :, None])        # [n, S, N_L]
        else:
            ok, t = medium_t(G, W.neg_inv_density[m], L[:, None, :], f32(FLT_MAX))
            ok, t = np.broadcast_to(ok, (n, tb.shape[1], N_L)), np.broadcast_to(t, (n, tb.shape[1], N_L))
            with np.errstate(all="ignore"):
                ok = ok & (t <= tb[:, :, None])  # th < tbest || (th == tbest && later entry): the media come in entry order
        ntb = np.where(ok, t, tb[:, :, None]).astype(f32).reshape(n, -1)
        nhit = np.where(ok, W.n_prims + m, hit[:, :, None]).reshape(n, -1)
        nvalid = (valid[:, :, None] & lv[:, None, :]).reshape(n, -1)
        tb, hit, valid = _strip(ntb, nhit, nvalid)
    p = np.zeros(tb.shape + (3,), f32)
    with np.errstate(all="ignore"):
        for m in range(W.n_media):
            sel = valid & (hit == W.n_prims + m)
            if sel.any():
                G = Gs[m]
                q = W.point_out(m, tuple((G["ro"][k][:, None] + G["rd"][k][:, None] * tb).astype(f32) for k in range(3)))  # Ray::at
                for k in range(3):
                    p[..., k] = np.where(sel, q[k], p[..., k])
    t = np.where(hit >= 0, tb, f32(0.0)).astype(f32)
    srt = np.sort(np.where(valid, hit, np.int64(-2)), axis=1)
    first = np.concatenate([np.ones((n, 1), bool), srt[:, 1:] != srt[:, :-1]], axis=1)
    n_hits = (first & (srt != -2)).sum(axis=1)
    return dict(hit=hit, t=t, valid=valid, p=p, n_hits=n_hits, intervals=Gs)


def element(S, hit, t):
    """the column of each ray's set whose (hit, t) equal the given ones bit for bit, -1 where there is none (t of a miss is not compared)"""
    same = S["valid"] & (S["hit"] == np.asarray(hit, np.int64)[:, None]) & ((bits(S["t"]) == bits(t)[:, None]) | (S["hit"] < 0))
    return np.where(same.any(axis=1), same.argmax(axis=1), -1)


def same_sets(A, B):
    """[n] bool: the two sets of a ray hold the same (hit, t) pairs"""
    def keys(S):
        k = (S["hit"] + 1) << 32 | bits(S["t"]).astype(np.int64)
        k = np.sort(np.where(S["valid"], k, np.int64(2 ** 62)), axis=1)
        return k
    ka, kb = keys(A), keys(B)
    w = max(ka.shape[1], kb.shape[1])
    pad = lambda k: np.concatenate([k, np.full((len(k), w - k.shape[1]), 2 ** 62, np.int64)], axis=1)
    return (pad(ka) == pad(kb)).all(axis=1)


def scalar_medium(W, m, o, d, xi, t_max):
    """ConstantMedium::hit of medium m for ONE world ray through tests/golden/np_ref.py (sphere_hit, rect_hit, translate_hit, rotate_y_hit,
    constant_medium_hit, host log): the scalar composition the vectorised restatement above is held to in tests/test_medium_ref_host.py.
    -> (t, p in the space of the ray the medium received) or None"""
    a = W.a

    def prim(i):
        if i < W.ns:
            c, r = np_ref.v3(a["sph_cx"][i], a["sph_cy"][i], a["sph_cz"][i]), f32(a["sph_r"][i])
            h = lambda ro, rd, t0, t1: np_ref.sphere_hit(c, r, ro, rd, t0, t1)
        else:
            k = i - W.ns
            axis, mn, mx = int(a["rect_axis"][k]), np_ref.v3(*a["rect_min"][3 * k:3 * k + 3]), np_ref.v3(*a["rect_max"][3 * k:3 * k + 3])
            h = lambda ro, rd, t0, t1: np_ref.rect_hit(axis, mn, mx, ro, rd, t0, t1)
        for x in _chain(a, W.prim_xform(i), W.med_xform[m]):
            q = tuple(f32(v) for v in a["xf_param"][4 * x:4 * x + 4])
            if int(a["xf_type"][x]) == 0:
                h = (lambda inner, off: lambda ro, rd, t0, t1: np_ref.translate_hit(off, inner, ro, rd, t0, t1))(h, q[:3])
            else:
                h = (lambda inner, s_, c_: lambda ro, rd, t0, t1: np_ref.rotate_y_hit(s_, c_, inner, ro, rd, t0, t1))(h, q[0], q[1])
        return h
    prims = [prim(int(i)) for i in W.boundary[m]]

    def boundary(ro, rd, t0, t1):  # HitableList::hit hitable.rs:117-132
        best = None
        for h in prims:
            r = h(ro, rd, t0, t1)
            if r is not None:
                best, t1 = r, r["t"]
        return best
    ro, rd = tuple(f32(x) for x in o), tuple(f32(x) for x in d)
    for x in reversed(_chain(a, W.med_xform[m])):
        q = tuple(f32(v) for v in a["xf_param"][4 * x:4 * x + 4])
        if int(a["xf_type"][x]) == 0:
            ro = np_ref.sub(ro, q[:3])
        else:
            s, c = q[0], q[1]
            ro, rd = (c * ro[0] - s * ro[2], ro[1], s * ro[0] + c * ro[2]), (c * rd[0] - s * rd[2], rd[1], s * rd[0] + c * rd[2])
    with np.errstate(all="ignore"):
        h = np_ref.constant_medium_hit(boundary, W.neg_inv_density[m], ro, rd, T_MIN, f32(t_max), f32(xi))
    return None if h is None else (h["t"], h["p"])
