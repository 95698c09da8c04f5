"""Float64 restatement of the reference's instance wrappers (hitable.rs:404-520) for one primitive's chain, read from an RtFlatScene.

`Translate::hit` moves the ray origin by -offset (hitable.rs:411); `RotateY::hit` maps origin and direction through
(x, z) -> (cos x - sin z, sin x + cos z) (hitable.rs:483-492) with the sin / cos RotateY::new stored in f32.  Taken in exact
arithmetic with those STORED values (no angle is re-derived), the world -> object map of a chain is affine, `object = A world + b`.
A RotateY level is cos/sin of an f32 pair, so it scales x and z by s = sqrt(sin^2 + cos^2), which is not 1: its exact inverse is
(x, z) -> (cos x + sin z, -sin x + cos z) / s^2.  The exact world region of an object-space sphere is therefore an ellipsoid (semi-axes
r / S in x and z, r in y, S = the product of the levels' s), and that of a rectangle the parallelogram through its mapped corners.

The hit tests take an f32 world ray, map it in float64 and test the primitive in object space (Sphere::hit hitable.rs:75-91,
XYRect::hit and its twins hitable.rs:250-270) without rounding.  They return a signed margin: how far inside (> 0) or outside (< 0)
the silhouette or the nearest edge the ray passes, in units of the primitive's own size."""
import numpy as np

NO_XFORM = 0xFFFFFFFF
T_MIN = 1e-3  # world_hit(.., 0.001, f32::MAX), main.rs:44


def chain(fs, prim):
    """The wrappers of primitive `prim` (spheres first, then rectangles), innermost first, as (type, f32 params[3])."""
    if prim < fs.n_spheres:
        x = fs.sph_xform[prim] if (fs.n_xforms and fs.sph_xform) else NO_XFORM
    else:
        x = fs.rect_xform[prim - fs.n_spheres] if (fs.n_xforms and fs.rect_xform) else NO_XFORM
    out = []
    while x != NO_XFORM:
        out.append((int(fs.xf_type[x]), np.array([fs.xf_param[4 * x + k] for k in range(3)], dtype=np.float32)))
        x = fs.xf_parent[x]
    return out


def _rot(q):
    sn, cs = float(q[0]), float(q[1])
    return np.array([[cs, 0.0, -sn], [0.0, 1.0, 0.0], [sn, 0.0, cs]])


def world_to_object(ch):
    """(A, b) with object = A @ world + b: the chain applied outermost first."""
    A, b = np.eye(3), np.zeros(3)
    for ty, q in reversed(ch):
        if ty == 0:
            b = b - q.astype(np.float64)
        else:
            M = _rot(q)
            A, b = M @ A, M @ b
    return A, b


def object_to_world(ch, p):
    """The exact inverse map of points p [..., 3] (innermost wrapper first: Translate adds its offset, RotateY applies R / s^2)."""
    p = np.array(p, dtype=np.float64)
    for ty, q in ch:
        if ty == 0:
            p = p + q.astype(np.float64)
        else:
            sn, cs = float(q[0]), float(q[1])
            s2 = cs * cs + sn * sn
            x, z = p[..., 0].copy(), p[..., 2].copy()
            p[..., 0] = (cs * x + sn * z) / s2
            p[..., 2] = (-sn * x + cs * z) / s2
    return p


def xz_scale(ch):
    """S = the product of sqrt(sin^2 + cos^2) over the RotateY levels: |A v| = S |v| for v in the xz-plane, y is kept."""
    S = 1.0
    for ty, q in ch:
        if ty == 1:
            S *= np.sqrt(float(q[0]) ** 2 + float(q[1]) ** 2)
    return S


def s2_minus_1(q):
    return float(q[0]) ** 2 + float(q[1]) ** 2 - 1.0


def intermediate_magnitude(ch, p):
    """The largest |coordinate| the points p take on their way through the chain (outermost first), world and object included:
    the scale at which an f32 evaluation of the chain rounds."""
    p = np.array(p, dtype=np.float64).reshape(-1, 3)
    m = np.abs(p).max(axis=1)
    for ty, q in reversed(ch):
        if ty == 0:
            p = p - q.astype(np.float64)
        else:
            p = p @ _rot(q).T
        m = np.maximum(m, np.abs(p).max(axis=1))
    return m


def fp32_object_ray(ch, o, d):
    """The ray as the kernels and the oracle map it (every operation rounded to f32 once, outermost wrapper first)."""
    f = np.float32
    o = np.array(o, dtype=f).reshape(-1, 3)
    d = np.array(d, dtype=f).reshape(-1, 3)
    for ty, q in reversed(ch):
        if ty == 0:
            o = (o - q.astype(f)).astype(f)
        else:
            sn, cs = f(q[0]), f(q[1])
            for v in (o, d):
                x = ((cs * v[:, 0]).astype(f) - (sn * v[:, 2]).astype(f)).astype(f)
                z = ((sn * v[:, 0]).astype(f) + (cs * v[:, 2]).astype(f)).astype(f)
                v[:, 0], v[:, 2] = x, z
    return o, d


class Prim:
    """One primitive of a flat scene with its chain: exact world region and exact hit tests."""

    def __init__(self, fs, prim):
        self.id = prim
        self.ch = chain(fs, prim)
        self.A, self.b = world_to_object(self.ch)
        self.S = xz_scale(self.ch)
        self.sphere = prim < fs.n_spheres
        if self.sphere:
            self.c = np.array([fs.sph_cx[prim], fs.sph_cy[prim], fs.sph_cz[prim]], dtype=np.float64)
            self.r = abs(float(fs.sph_r[prim]))
            self.size = self.r
        else:
            i = prim - fs.n_spheres
            self.ax = int(fs.rect_axis[i])
            mn = np.array([fs.rect_min[3 * i + k] for k in range(3)], dtype=np.float64)
            mx = np.array([fs.rect_max[3 * i + k] for k in range(3)], dtype=np.float64)
            self.k = mn[self.ax]
            self.ua, self.va = (1 if self.ax == 0 else 0), (1 if self.ax == 2 else 2)
            self.lo, self.hi = mn, mx
            self.size = max(mx[self.ua] - mn[self.ua], mx[self.va] - mn[self.va])

    def in_plane_fp32(self, o, d):
        """True where the f32 object-space ray of a rectangle lies in its plane (XYRect::hit then divides 0 by 0)."""
        if self.sphere:
            return np.zeros(len(o), dtype=bool)
        oo, dd = fp32_object_ray(self.ch, o, d)
        return (dd[:, self.ax] == 0) & (oo[:, self.ax] == np.float32(self.k))

    # -- exact world region ------------------------------------------------------------------------------------------------------
    def corners(self):
        """Object-space corners of a rectangle [4, 3]."""
        out = []
        for cu in (self.lo[self.ua], self.hi[self.ua]):
            for cv in (self.lo[self.va], self.hi[self.va]):
                p = np.zeros(3)
                p[self.ax], p[self.ua], p[self.va] = self.k, cu, cv
                out.append(p)
        return np.array(out)

    def world_centre(self):
        return object_to_world(self.ch, self.c if self.sphere else self.corners().mean(axis=0))

    def world_box(self):
        """(lo[3], hi[3]) of the exact world region (the ellipsoid's box, or the box of the mapped corners)."""
        if self.sphere:
            wc = object_to_world(self.ch, self.c)
            h = np.array([self.r / self.S, self.r, self.r / self.S])
            return wc - h, wc + h
        w = object_to_world(self.ch, self.corners())
        return w.min(axis=0), w.max(axis=0)

    def world_ball(self):
        """(centre, radius) of a ball around the exact world region."""
        if self.sphere:
            return object_to_world(self.ch, self.c), self.r * max(1.0, 1.0 / self.S)
        w = object_to_world(self.ch, self.corners())
        c = w.mean(axis=0)
        return c, float(np.linalg.norm(w - c, axis=1).max())

    # -- exact hit tests ---------------------------------------------------------------------------------------------------------
    def to_object(self, o, d):
        o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
        d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
        return o @ self.A.T + self.b, d @ self.A.T

    def exact_hit(self, o, d, t_min=T_MIN):
        """For f32 world rays (o, d) [n, 3]: (margin [n], t [n]).  margin > 0: the ray meets the primitive in exact arithmetic,
        by that fraction of its size inside the silhouette / the nearest edge; < 0: it passes that far outside.  t: the root
        Sphere::hit / XYRect::hit would take in exact arithmetic (inf where there is none in [t_min, inf))."""
        oo, dd = self.to_object(o, d)
        if self.sphere:
            oc = oo - self.c
            a = np.einsum("ij,ij->i", dd, dd)
            tc = -np.einsum("ij,ij->i", oc, dd) / a
            close = oc + tc[:, None] * dd
            dist = np.linalg.norm(close, axis=1)
            margin = (self.r - dist) / self.r
            h = np.sqrt(np.maximum(self.r * self.r - dist * dist, 0.0) / a)
            t0, t1 = tc - h, tc + h
            t = np.where(t0 >= t_min, t0, np.where(t1 >= t_min, t1, np.inf))
            t = np.where(margin >= 0, t, np.inf)
            return margin, t
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (self.k - oo[:, self.ax]) / dd[:, self.ax]
            p = oo + t[:, None] * dd
            m = np.minimum.reduce([p[:, self.ua] - self.lo[self.ua], self.hi[self.ua] - p[:, self.ua],
                                   p[:, self.va] - self.lo[self.va], self.hi[self.va] - p[:, self.va]]) / self.size
        ok = np.isfinite(t) & (t >= t_min)
        margin = np.where(ok, np.nan_to_num(m, nan=-np.inf), -np.inf)
        return margin, np.where(ok & (margin >= 0), t, np.inf)

    def rounding_scale(self, o, d, t):
        """An upper bound of how far (in units of the primitive's size) an f32 evaluation of the chain and of the primitive's own
        test can move the ray at the hit: per level, a few ulp of the largest magnitude the origin and the hit point take there (1 per
        Translate, 12 per RotateY, as rt_scene_upload's error model), the primitive's own arithmetic at its object-space magnitude, and
        for a sphere the cancellation of |oc|^2 - r^2 (hitable.rs:79-83)."""
        o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
        d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
        tt = np.where(np.isfinite(t), t, 0.0)
        p = o + tt[:, None] * d
        e = np.zeros(len(o))
        a, b = o.copy(), p.copy()
        for ty, q in reversed(self.ch):
            m_in = np.maximum(np.abs(a).max(axis=1), np.abs(b).max(axis=1))
            if ty == 0:
                a, b = a - q.astype(np.float64), b - q.astype(np.float64)
            else:
                a, b = a @ _rot(q).T, b @ _rot(q).T
            m = np.maximum(m_in, np.maximum(np.abs(a).max(axis=1), np.abs(b).max(axis=1)))
            e = e + (1.0 if ty == 0 else 12.0) * m
        m_obj = np.maximum(np.abs(a).max(axis=1), np.abs(b).max(axis=1))
        e = 1.7321 * 2.0 ** -24 * (e + 8.0 * m_obj) / self.size
        if self.sphere:
            oc2 = ((a - self.c) ** 2).sum(axis=1)
            e = e + 8.0 * 2.0 ** -24 * oc2 / (self.r * self.r)
        return e

    def chain_scale(self):
        """The rounding scale of the chain for rays that start among its own points (rt_scene_upload's model), in units of the
        primitive's size: what a margin has to exceed before f32 can no longer move the ray across the edge."""
        pts = self.corners() if not self.sphere else self.c[None] + self.r * np.vstack([np.eye(3), -np.eye(3)])
        w = object_to_world(self.ch, pts)
        return float(self.rounding_scale(w[:1], np.array([[0.0, 0.0, 1.0]]), np.zeros(1))[0]) * 2.0


def primitives(fs):
    return [Prim(fs, i) for i in range(fs.n_spheres + fs.n_rects)]
