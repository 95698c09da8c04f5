"""First-hit features (rtow_mi355x.h "First-hit features") restated without the kernel that computes them: the reference of
tests/test_features.py.

Nothing of k_features is used.  A feature sample is named by (pixel, sample) alone.  Its primary ray is helpers.primary_rays (the
pinhole) or lens_ref.lens_rays (a lens), its key helpers.path_keys, its time motion_ref.path_time.  The closest hit comes from
Renderer.debug_bounce(o, d, keys, depth=0, FLAG_BRUTE_FORCE): the single-kernel list walk, which the suite holds per ray to the oracle and
to the numpy references under every set.  From it: the hit index, t, and — where the material hands its first texture on unchanged — the
albedo: Diffuse and Isotropic return it as their attenuation, Emission as its radiance.  For every other tag the albedo is read from the
scene description: the constant colour of the first texture (tags 2, 6 .. 11: their attenuation is the texture times a lobe, so the tests
use constant textures there), the material colour (Metal), 1 (Dielectric, DisneyClearcoat), 0 (an unknown tag).

The normal is computed here, in numpy float32, one rounding per operation in the order of hitable.rs (glam: dot = (xx + yy) + zz):
the world ray through the wrappers of the primitive, outermost first (Translate hitable.rs:411, RotateY 483-492); p = o + d t in object
space; the outward normal (p - c) / r of a sphere (c at the path's time under a motion set), the +axis unit vector of a rectangle, the
set-up normal of a planar primitive (quad_ref.setup); set_face_normal; then from the innermost wrapper out: RotateY rotates the normal
(hitable.rs:495-498) and applies set_face_normal again with the direction its own child received (hitable.rs:505), Translate leaves it.
A medium's sample has normal 0.  Every case is exact: no comparison in tests/test_features.py needs a rounding bound.

The record is then summed as the header states it: f32 sums of a and n, one addition per sample in ascending sample order; f64 moments
a2 += (ax ax + ay ay) + az az, n2 likewise, z1 += z, z2 += z z on the converted f32 values; the counters."""
import numpy as np

import lens_ref
import motion_ref
import quad_ref
from helpers import primary_rays

f32 = np.float32
NONE = 0xFFFFFFFF
FLAG_BRUTE_FORCE = 1
TEX0_USERS = (0, 1, 2, 5, 6, 7, 8, 9, 10, 11)
PIXEL = np.dtype([("albedo", "<f4", (3,)), ("n_f", "<u4"), ("normal", "<f4", (3,)), ("n_h", "<u4"), ("a2", "<f8"), ("n2", "<f8"),
                  ("z1", "<f8"), ("z2", "<f8")])


def _dot(a, b):
    return ((a[0] * b[0]).astype(f32) + (a[1] * b[1]).astype(f32)).astype(f32) + (a[2] * b[2]).astype(f32)


def _xform_ray(a, x, o, d):
    q = a["xf_param"][4 * x:4 * x + 4].astype(f32)
    if int(a["xf_type"][x]) == 0:
        return ((o[0] - q[0]).astype(f32), (o[1] - q[1]).astype(f32), (o[2] - q[2]).astype(f32)), d
    s, c = q[0], q[1]
    rot = lambda v: (((c * v[0]).astype(f32) - (s * v[2]).astype(f32)).astype(f32), v[1], ((s * v[0]).astype(f32) + (c * v[2]).astype(f32)).astype(f32))
    return rot(o), rot(d)


def _chain(a, x):
    """the wrappers of a primitive from the innermost one outwards"""
    out = []
    x = int(x)
    while x != NONE:
        out.append(x)
        x = int(a["xf_parent"][x])
    return out


def clamp01(a):
    """per channel: NaN -> 0, then the clamp to [0, 1]"""
    a = np.asarray(a, f32)
    return np.where(np.isnan(a), f32(0), np.minimum(np.maximum(a, f32(0)), f32(1))).astype(f32)


class World:
    """What the reference reads of the scene description, of a motion set (spheres, center1, shutter) and of a planar set (q, u, v, kind,
    mat)."""

    def __init__(self, scene, motion=None, quads=None):
        self.a = a = scene.arrays()
        fs = scene.flat
        self.ns, self.nr, self.n_media = int(fs.n_spheres), int(fs.n_rects), int(fs.n_media)
        self.n_prims = self.ns + self.nr
        self.pbase = self.n_prims + self.n_media
        self.c0 = np.stack([a["sph_cx"], a["sph_cy"], a["sph_cz"]], axis=1).astype(f32) if self.ns else np.zeros((0, 3), f32)
        self.c1, self.shutter = {}, None
        if motion is not None:
            idx, c1, self.shutter = motion
            self.c1 = {int(i): np.asarray(c, f32) for i, c in zip(idx, np.asarray(c1, f32).reshape(-1, 3))}
        self.quads = None
        if quads is not None:
            q, u, v, kind, mat = quads
            self.quads = dict(normal=quad_ref.setup(q, u, v)[0], mat=np.asarray(mat, np.int64))

    def material(self, h):
        a = self.a
        if h >= self.pbase:
            return int(self.quads["mat"][h - self.pbase])
        if h >= self.n_prims:
            return int(a["med_mat"][h - self.n_prims])
        return int(a["sph_mat"][h]) if h < self.ns else int(a["rect_mat"][h - self.ns])

    def described_albedo(self, h):
        """the albedo of entry h where the scene description gives it: [3] f32, or None (the hook's output gives it)"""
        a = self.a
        m = self.material(h)
        tag = int(a["mat_type"][m])
        if tag in (0, 1, 5):
            return None
        if tag in TEX0_USERS:
            tex = int(a["mat_tex0"][m])
            assert int(a["tex_type"][tex]) == 0, "tags 2, 6 .. 11 are held over constant textures"
            return a["tex_color0"][3 * tex:3 * tex + 3].astype(f32)
        if tag == 3:
            return a["mat_color"][3 * m:3 * m + 3].astype(f32)
        return np.ones(3, f32) if tag in (4, 12) else np.zeros(3, f32)

    def normal(self, h, o, d, t, tm):
        """the world-space, face-forwarded normal of entry h for the rays (o, d) [m, 3] hit at t [m] (tm [m]: their times, or None)"""
        a = self.a
        m = len(t)
        wo, wd = tuple(o[:, k] for k in range(3)), tuple(d[:, k] for k in range(3))
        if h >= self.pbase:
            on = tuple(np.full(m, x, f32) for x in self.quads["normal"][h - self.pbase])
            front = _dot(wd, on) < f32(0)
            return np.stack([np.where(front, c, -c) for c in on], axis=1).astype(f32)
        if h >= self.n_prims:
            return np.zeros((m, 3), f32)
        chain = _chain(a, (a["sph_xform"][h] if len(a["sph_xform"]) else NONE) if h < self.ns
                       else (a["rect_xform"][h - self.ns] if len(a["rect_xform"]) else NONE))
        ro, rd = wo, wd
        for w in reversed(chain):
            ro, rd = _xform_ray(a, w, ro, rd)
        if h < self.ns:
            c = np.tile(self.c0[h], (m, 1))
            if h in self.c1:
                c = motion_ref.center_at(self.c0[h], self.c1[h], tm)
            r = a["sph_r"][h].astype(f32)
            p = tuple((ro[k] + (rd[k] * t).astype(f32)).astype(f32) for k in range(3))
            on = tuple(((p[k] - c[:, k]).astype(f32) / r).astype(f32) for k in range(3))
        else:
            axis = int(a["rect_axis"][h - self.ns])
            on = tuple(np.full(m, 1.0 if k == axis else 0.0, f32) for k in range(3))
        front = _dot(rd, on) < f32(0)
        n = tuple(np.where(front, c, -c).astype(f32) for c in on)
        for k, w in enumerate(chain):
            if int(a["xf_type"][w]) == 0:
                continue
            q = a["xf_param"][4 * w:4 * w + 4].astype(f32)
            s, c = q[0], q[1]
            n = (((c * n[0]).astype(f32) + (s * n[2]).astype(f32)).astype(f32), n[1], ((-s * n[0]).astype(f32) + (c * n[2]).astype(f32)).astype(f32))
            ok, dk = wo, wd
            for j in reversed(range(k, len(chain))):  # the ray this wrapper handed to its child
                ok, dk = _xform_ray(a, chain[j], ok, dk)
            front = _dot(dk, n) < f32(0)
            n = tuple(np.where(front, x, -x).astype(f32) for x in n)
        return np.stack(n, axis=1).astype(f32)


def first_hits(r, scene, p, samples, lens=None, motion=None, quads=None):
    """The feature samples of the absolute sample indices `samples` of every pixel of the frame `p` on Renderer `r`, which holds the
    uploaded scene and its sets -> dict(a [S, ny, nx, 3], n [S, ny, nx, 3], hit [S, ny, nx] bool, z [S, ny, nx], index [S, ny, nx])."""
    nx, ny = int(p.nx), int(p.ny)
    samples = np.asarray(samples, np.int64)
    ss, jj, ii = np.meshgrid(samples, np.arange(ny), np.arange(nx), indexing="ij")
    s, j, i = ss.ravel(), jj.ravel(), ii.ravel()
    if lens is not None and f32(lens[0]) > 0:
        o, d, keys = lens_ref.lens_rays(scene.camera, p, i, j, s, lens[0], lens[1])
    else:
        o, d, keys = primary_rays(scene, p, i, j, s)
    w = World(scene, motion, quads)
    tm = motion_ref.path_time(keys, *w.shutter) if w.shutter is not None else None
    out = r.debug_bounce(o, d, keys, depth=0, flags=FLAG_BRUTE_FORCE)
    hit, t = out["hit"].astype(np.int64), out["t"].astype(f32)
    a = np.ones((len(s), 3), f32)
    n = np.zeros((len(s), 3), f32)
    with np.errstate(all="ignore"):
        for h in np.unique(hit[hit >= 0]):
            sel = hit == h
            h = int(h)
            desc = w.described_albedo(h)
            if desc is not None:
                a[sel] = clamp01(desc)
            else:
                tag = int(w.a["mat_type"][w.material(h)])
                a[sel] = clamp01(out["radiance"][sel] if tag == 0 else out["attenuation"][sel])
            n[sel] = w.normal(h, o[sel], d[sel], t[sel], None if tm is None else tm[sel])
    shape = (len(samples), ny, nx)
    return dict(a=a.reshape(shape + (3,)), n=n.reshape(shape + (3,)), hit=(hit >= 0).reshape(shape), z=np.where(hit >= 0, t, f32(0)).astype(f32).reshape(shape),
                index=hit.reshape(shape))


def contributing(first, n, stride):
    """the absolute indices of the samples first .. first + n - 1 that take a feature sample"""
    return np.array([s for s in range(first, first + n) if s % stride == 0], np.int64)


def accumulate(fh, plane=None, active=None):
    """Adds the feature samples `fh` (first_hits, in ascending sample order) onto `plane` [ny, nx] of PIXEL (zeros where None) for the
    pixels of `active` [ny, nx] bool (all where None); returns the new plane."""
    S, ny, nx = fh["hit"].shape
    out = np.zeros((ny, nx), PIXEL) if plane is None else plane.copy()
    act = np.ones((ny, nx), bool) if active is None else active
    for k in range(S):
        a, n, hit, z = fh["a"][k], fh["n"][k], fh["hit"][k] & act, fh["z"][k].astype(np.float64)
        out["albedo"] = np.where(act[..., None], (out["albedo"] + a).astype(f32), out["albedo"])
        out["normal"] = np.where(act[..., None], (out["normal"] + n).astype(f32), out["normal"])
        out["n_f"] += act.astype(np.uint32)
        out["n_h"] += hit.astype(np.uint32)
        a64, n64 = a.astype(np.float64), n.astype(np.float64)
        out["a2"] = np.where(act, out["a2"] + ((a64[..., 0] * a64[..., 0] + a64[..., 1] * a64[..., 1]) + a64[..., 2] * a64[..., 2]), out["a2"])
        out["n2"] = np.where(act, out["n2"] + ((n64[..., 0] * n64[..., 0] + n64[..., 1] * n64[..., 1]) + n64[..., 2] * n64[..., 2]), out["n2"])
        out["z1"] = np.where(hit, out["z1"] + z, out["z1"])
        out["z2"] = np.where(hit, out["z2"] + z * z, out["z2"])
    return out


def _var_of_mean(s2, sq, count):
    n = count.astype(np.float64)
    with np.errstate(all="ignore"):
        v = (s2 - sq / n) / (n - 1.0)
        v = np.where(v < 0.0, 0.0, v) / n
    return np.where(count >= 2, v, 0.0).astype(f32)


def read_out(plane):
    """rt_accum_read_features of a plane of PIXEL: dict(albedo, normal, depth, hit, var) in f32"""
    nf, nh = plane["n_f"], plane["n_h"]
    N = nf.astype(f32)
    with np.errstate(all="ignore"):
        albedo = np.where(nf[..., None] > 0, (plane["albedo"] / N[..., None]).astype(f32), f32(0)).astype(f32)
        normal = np.where(nf[..., None] > 0, (plane["normal"] / N[..., None]).astype(f32), f32(0)).astype(f32)
        depth = np.where(nh > 0, (plane["z1"] / nh.astype(np.float64)).astype(f32), f32(0)).astype(f32)
        hit = np.where(nf > 0, (nh.astype(f32) / N).astype(f32), f32(0)).astype(f32)
    sq = lambda v: (v[..., 0].astype(np.float64) ** 2 + v[..., 1].astype(np.float64) ** 2) + v[..., 2].astype(np.float64) ** 2
    var = np.stack([_var_of_mean(plane["a2"], sq(plane["albedo"]), nf), _var_of_mean(plane["n2"], sq(plane["normal"]), nf),
                    _var_of_mean(plane["z2"], plane["z1"] * plane["z1"], nh)], axis=-1)
    return dict(albedo=albedo, normal=normal, depth=depth, hit=hit, var=var)


def same_bits(x, y):
    """two planes of PIXEL (or two arrays of one dtype), byte for byte"""
    return np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


# ---- the feature-guided filter (rtow_mi355x.h "The feature-guided filter"), on top of denoise_ref -----------------------------------------
USE_ALBEDO, USE_NORMAL, USE_DEPTH = 1, 2, 4
INV64 = f32(0.015625)


def guide(use=7, k=0.6, tau=1e-3, demodulate=False):
    """the RtFeatureGuide as a dict: k and tau one value or (albedo, normal, depth)"""
    k3 = tuple(k) if np.ndim(k) else (k,) * 3
    t3 = tuple(tau) if np.ndim(tau) else (tau,) * 3
    return dict(use=int(use), k=tuple(f32(x) for x in k3), tau=tuple(f32(x) for x in t3), demodulate=bool(demodulate))


def filter_inputs(plane):
    """(feat_mean [rows, nx, 7], feat_var [rows, nx, 3]) of a plane of PIXEL: read_out's values, NaN for all ten where n_f < 2"""
    out = read_out(plane)
    fm = np.concatenate([out["albedo"], out["normal"], out["depth"][..., None]], axis=-1).astype(f32)
    fv = out["var"].astype(f32).copy()
    none = plane["n_f"] < 2
    fm[none], fv[none] = np.nan, np.nan
    return fm, fv


def demodulation_albedo(fm):
    a = fm[..., :3]
    return np.where(a > INV64, a, INV64).astype(f32)  # (a NaN: 1/64)


def demodulate(c, y, v, fm):
    a = demodulation_albedo(fm)
    Ya = ((f32(0.2126) * a[..., 0]).astype(f32) + (f32(0.7152) * a[..., 1]).astype(f32)).astype(f32) + (f32(0.0722) * a[..., 2]).astype(f32)
    with np.errstate(all="ignore"):
        return (c / a).astype(f32), (y / Ya).astype(f32), (v / (Ya * Ya).astype(f32)).astype(f32), a


def denoise_features(c, y, v, feat_mean, feat_var, radius, patch, strength, g):
    """The filter of the header in numpy f32, one IEEE operation per step in the header's order: denoise_ref.nlm's loop (the same patch
    distance from the same operands) with the feature distances of every pair beside D_c.  Returns the filtered [rows, nx, 3]."""
    import denoise_ref
    EPS = denoise_ref.EPS
    c, y, v = np.asarray(c, f32), np.asarray(y, f32), np.asarray(v, f32)
    fm, fv = np.asarray(feat_mean, f32), np.asarray(feat_var, f32)
    a_p = None
    if g["demodulate"]:
        c, y, v, a_p = demodulate(c, y, v, fm)
    (rows, nx), R, F, k = c.shape[:2], int(radius), int(patch), f32(strength)
    k2, cnt = f32(k * k), f32((2 * F + 1) * (2 * F + 1))
    (ys, xs), (ye, xe) = np.mgrid[0:rows, 0:nx], np.mgrid[-F:rows + F, -F:nx + F]
    at = lambda a, yy, xx: a[np.clip(yy, 0, rows - 1), np.clip(xx, 0, nx - 1)]
    kf2 = [f32(x * x) for x in g["k"]]
    floor_z = (g["tau"][2] * (fm[..., 6] * fm[..., 6]).astype(f32)).astype(f32)
    den, num = np.zeros((rows, nx), f32), np.zeros((rows, nx, 3), f32)
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < nx)
                diff, va, vb = at(y, ye, xe) - at(y, ye + dy, xe + dx), at(v, ye, xe), at(v, ye + dy, xe + dx)
                e = (diff * diff - (va + np.where(vb < va, vb, va))) / (EPS + k2 * (va + vb))
                S = np.zeros((rows, nx), f32)
                for oy in range(F + F + 1):
                    row = np.zeros((rows, nx), f32)
                    for ox in range(F + F + 1):
                        row = row + e[oy:oy + rows, ox:ox + nx]
                    S = S + row
                D = S / cnt
                m = np.where(D < 0, f32(0), D)
                bad = np.zeros((rows, nx), bool)
                fq, vq = at(fm, qy, qx), at(fv, qy, qx)
                for bit, comps, j in ((USE_ALBEDO, (0, 1, 2), 0), (USE_NORMAL, (3, 4, 5), 1), (USE_DEPTH, (6,), 2)):
                    if not g["use"] & bit:
                        continue
                    sq = [((fm[..., i] - fq[..., i]).astype(f32) ** 2).astype(f32) for i in comps]
                    s2 = ((sq[0] + sq[1]).astype(f32) + sq[2]).astype(f32) if len(sq) == 3 else sq[0]
                    vp_, vq_ = fv[..., j], vq[..., j]
                    vmin = np.where(vq_ < vp_, vq_, vp_)
                    vs = (vp_ + vq_).astype(f32)
                    floor = floor_z if j == 2 else np.full((rows, nx), g["tau"][j], f32)
                    vmax = np.where(vs > floor, vs, floor)
                    d = ((s2 - (vp_ + vmin).astype(f32)).astype(f32) / (EPS + (kf2[j] * vmax).astype(f32)).astype(f32)).astype(f32)
                    bad |= np.isnan(d)
                    m = np.where(d > m, d, m)
                u = f32(1) - f32(0.25) * m
                u = np.where(u > 0, u, f32(0))
                u = np.where(bad, f32(0), u).astype(f32)
                w = (u * u) * (u * u)
                use = inside & (u != 0)
                den = np.where(use, den + w, den)
                num = np.where(use[..., None], num + w[..., None] * at(c, qy, qx), num)
        out = np.where((den == 0)[..., None], c, num / den[..., None]).astype(f32)
        if a_p is not None:
            out = (out * a_p).astype(f32)
    assert out.dtype == f32 and den.dtype == f32 and num.dtype == f32
    return out


def step_plane(nx=24, rows=12, noise=0.5, seed=3):
    """The designed plane: one flat colour times an albedo that steps from 0.2 to 0.8 in the middle column, under colour noise large
    against the step's luminance difference, so that the colour guide alone blurs the step; the features are exact (variance 0 but for a
    small floor), normal and depth constant.  Returns (truth, c, y, v, feat_mean, feat_var)."""
    rng = np.random.default_rng(seed)
    albedo = np.where(np.arange(nx)[None, :] < nx // 2, 0.2, 0.8) * np.ones((rows, 1))
    truth = (albedo[..., None] * np.array([0.9, 0.8, 0.7])).astype(f32)
    c = (truth * (1.0 + noise * rng.standard_normal((rows, nx, 1)))).astype(f32)
    lum = lambda x: 0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]
    y = lum(c).astype(f32)
    v = ((noise * lum(truth)) ** 2).astype(f32)  # the variance of the mean the noise was drawn with
    fm = np.zeros((rows, nx, 7), f32)
    fm[..., 0:3] = albedo[..., None]
    fm[..., 5], fm[..., 6] = 1.0, 10.0
    fv = np.full((rows, nx, 3), 1e-6, f32)
    return truth, c, y, v, fm, fv
