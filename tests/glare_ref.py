"""Reference for the glare of rtow_mi355x.h ("Glare") in numpy: f32 step by step, every operation one IEEE operation in the header's order
(numpy's element-wise operators never fuse), on top of denoise_multiscale_ref.down / up_add and display_ref.luminance, which are imported
and left as they are.  The kernels of csrc/rt_glare.h are held to glare() bit for bit.  glare64() evaluates the same formulas in f64 —
the same taps, weights and border rule, no f32 rounding — for the bounds the host tests derive."""
import types

import numpy as np

import denoise_multiscale_ref as ms
import display_ref

F32, F64 = np.float32, np.float64
MAX_LEVELS = 8
CEILING = F32(2.0 ** 64)
U24 = 2.0 ** -24  # the relative error bound of one f32 rounding (normal range)


def make(amount=0.1, spread=0.7, threshold=0.0, levels=6):
    """A glare for this module alone (the attributes of an RtGlare)."""
    return types.SimpleNamespace(amount=F32(amount), spread=F32(spread), threshold=F32(threshold), levels=int(levels))


def effective_levels(nx, rows, levels):
    """Le = min(levels, the first level whose larger side is 1); 0 for a 1 x 1 frame."""
    le = 0
    while le < levels and max(nx, rows) > 1:
        nx, rows = ms.level_size(nx, rows, 1)
        le += 1
    return le


def weights(spread, le, dtype=F32):
    """[ŵ_1 .. ŵ_Le]: w_1 = 1, w_{l+1} = w_l * spread, W = ((w_1 + w_2) + ..) in index order, ŵ_l = w_l / W; every operation in `dtype`."""
    w, cur = [], dtype(1)
    for _ in range(le):
        w.append(cur)
        cur = dtype(cur * dtype(spread))
    total = w[0] if w else dtype(1)
    for v in w[1:]:
        total = dtype(total + v)
    return [dtype(v / total) for v in w]


def sanitise(c):
    c = np.asarray(c, F32)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(c) & (c > 0), np.minimum(c, CEILING), F32(0)).astype(F32)


def bright(s, threshold):
    """b of the sanitised image s."""
    if F32(threshold) == 0:
        return s
    with np.errstate(all="ignore"):
        Y = display_ref.luminance(s)
        t = F32(threshold)
        k = np.where(Y > t, (Y - t) / np.where(Y > t, Y, F32(1)), F32(0)).astype(F32)
        b = s * k[..., None]
    assert b.dtype == F32
    return b


def glare(c, g):
    """(out [rows, nx, 3] f32, info) of the image c [rows, nx, 3] in the call's row order under the glare g.  info: levels (Le),
    coarse_nx, coarse_rows, and the intermediate s, b, d (list, d[0] = b) and u (list, u[0] = B)."""
    c = np.ascontiguousarray(c, F32)
    rows, nx = c.shape[:2]
    le = effective_levels(nx, rows, g.levels)
    s = sanitise(c)
    b = bright(s, g.threshold)
    fin = np.isfinite(c).all(axis=-1)
    d = [b]
    for _ in range(le):
        d.append(ms.down(d[-1]))
    info = {"levels": le, "coarse_nx": d[-1].shape[1], "coarse_rows": d[-1].shape[0], "s": s, "b": b, "d": d}
    if le == 0:
        out = np.where(fin[..., None], s, c).astype(F32)
        info["u"] = [b]
        return out, info
    w = weights(g.spread, le)
    u = [None] * (le + 1)
    with np.errstate(all="ignore"):
        u[le] = w[le - 1] * d[le]
        for l in range(le - 1, 0, -1):
            u[l] = ms.up_add(w[l - 1] * d[l], u[l + 1])
        u[0] = B = ms.up_add(np.zeros_like(b), u[1])  # (+0 + U: U itself, bit for bit, but for a -0, which no sum of non-negative terms gives)
        a = F32(g.amount)
        out = (s - a * b) + a * B
    assert out.dtype == F32 and all(x.dtype == F32 for x in u)
    info["u"] = u
    return np.where(fin[..., None], out, c).astype(F32), info


def _down64(a):
    rows, nx = a.shape[:2]
    nx1, rows1 = ms.level_size(nx, rows, 1)
    t = np.zeros((2 * rows1, 2 * nx1, 3), F64)
    t[:rows, :nx] = a
    ky = 1 + (2 * np.arange(rows1) + 1 < rows)
    kx = 1 + (2 * np.arange(nx1) + 1 < nx)
    return ((t[0::2, 0::2] + t[0::2, 1::2]) + (t[1::2, 0::2] + t[1::2, 1::2])) / (ky[:, None] * kx[None, :])[..., None]


def _up64(e, nx, rows):
    rows1, nx1 = e.shape[:2]
    y, x = np.mgrid[0:rows, 0:nx]
    X, Y = x >> 1, y >> 1
    X2 = np.clip(X + np.where(x & 1, 1, -1), 0, nx1 - 1)
    Y2 = np.clip(Y + np.where(y & 1, 1, -1), 0, rows1 - 1)
    return (0.5625 * e[Y, X] + 0.1875 * e[Y, X2]) + (0.1875 * e[Y2, X] + 0.0625 * e[Y2, X2])


def glare64(c, g):
    """The same formulas in f64 on a finite image (the f32 inputs and parameters, exact products and sums up to f64's own rounding)."""
    c = np.asarray(c, F32)
    assert np.isfinite(c).all()
    rows, nx = c.shape[:2]
    le = effective_levels(nx, rows, g.levels)
    s = sanitise(c).astype(F64)
    if le == 0:
        return s
    b = s
    if F32(g.threshold) != 0:
        Y = (F64(F32(0.2126)) * s[..., 0] + F64(F32(0.7152)) * s[..., 1]) + F64(F32(0.0722)) * s[..., 2]
        t = F64(F32(g.threshold))
        b = s * np.where(Y > t, (Y - t) / np.where(Y > t, Y, 1.0), 0.0)[..., None]
    d = [b]
    for _ in range(le):
        d.append(_down64(d[-1]))
    w = weights(F64(F32(g.spread)), le, F64)
    u = w[le - 1] * d[le]
    for l in range(le - 1, 0, -1):
        u = w[l - 1] * d[l] + _up64(u, d[l].shape[1], d[l].shape[0])
    B = _up64(u, nx, rows)
    a = F64(F32(g.amount))
    return (s - a * b) + a * B


def rounding_bound(le):
    """R with |glare(c) - glare64(c)| <= R * (glare64(c) + s) per value, on a finite image under threshold 0 (b = s) and away from
    underflow, derived from the f32 operations on the longest path to `out`.  Each rounds once with a relative error <= u = 2^-24, and a
    sum of non-negative terms has at most the largest relative error of its terms, plus its own rounding:
      ŵ_l: w_l carries l - 1 roundings, W those of its terms (<= Le - 1) and Le - 1 additions, the quotient one more: <= 3 Le;
      d_l: per level (t00 + t10), then + (t01 + t11) — two roundings in sequence; the scale is a power of two, exact: 2 l;
      u_Le = ŵ_Le d_Le: 3 Le + 2 Le + 1;
      u_l = ŵ_l d_l + U(u_{l+1}): U is a product, the inner and the outer addition (3), then the sum (1): 4 more per level, so u_1 carries
        5 Le + 1 + 4 (Le - 1) = 9 Le - 3, B = U(u_1) 9 Le, a B 9 Le + 1;
      s - a b is the one difference: a b <= s is off by <= u a b, the difference rounds once: <= u s in absolute terms;
      the final sum rounds once more.
    In all |error| <= (9 Le + 2) u a B + u s + u out <= (9 Le + 3) u (out + s); R takes 9 Le + 4 and 1 % for the second-order terms
    ((1 + u)^n <= 1 + 1.01 n u for n <= 100) and for glare64's own f64 roundings."""
    return 1.01 * (9 * le + 4) * U24


# ---- the planes of the tests --------------------------------------------------------------------------------------------------------------
# 1 x 1: Le = 0; 1 x 9, 5 x 1: one-pixel sides; 2 x 2: one level; 7 x 13, 33 x 17: odd at several levels; 64 x 64: even throughout, two
# tile rows of the fused chain; 257 x 129: odd at every level, crosses a 256-thread block, ends at 2 x 1; 300 x 200: tile edges of the
# fused chain inside the frame (64 x 16 tiles: 4.7 x 12.5 of them)
FRAMES = ((1, 1), (1, 9), (5, 1), (2, 2), (7, 13), (33, 17), (64, 64), (257, 129), (300, 200))


def constant_plane(nx, rows):
    return np.full((rows, nx, 3), (0.75, 0.3, 1.5), F32) * np.ones((rows, nx, 1), F32)


def impulse_plane(nx, rows):
    """Black but for impulses of different colours at the centre, in the four corners and in the last row (odd-indexed where rows is even:
    rows - 1) at a third of the width."""
    img = np.zeros((rows, nx, 3), F32)
    img[rows // 2, nx // 2] = (1000.0, 600.0, 250.0)
    img[0, 0] = (3.0, 0.0, 0.0)
    img[0, nx - 1] = (0.0, 5.0, 0.0)
    img[rows - 1, 0] = (0.0, 0.0, 7.0)
    img[rows - 1, nx - 1] = (11.0, 13.0, 17.0)
    img[rows - 1, nx // 3] += F32(19.0)
    return img


def random_plane(nx, rows, seed=23):
    """Log-uniform over 12 octaves, with NaN, +-inf, negative, > 2^64 and -0.0 pixels sprinkled in (whole pixels and single channels)."""
    rng = np.random.default_rng([seed, nx, rows])
    img = np.exp2(rng.uniform(-6, 6, (rows, nx, 3))).astype(F32)
    flat = img.reshape(-1, 3)
    n = flat.shape[0]
    specials = (np.nan, np.inf, -np.inf, -2.5, 2.0 ** 70, -0.0, np.finfo(F32).max, 2.0 ** 64, float(np.nextafter(F32(2.0 ** 64), F32(np.inf))))
    for k, v in enumerate(specials):
        if n > k:
            flat[(k * 7919 + 3) % n, k % 3] = v
        if n > 64:
            flat[(k * 104729 + 11) % n] = v
    return img


PLANES = (("constant", constant_plane), ("impulses", impulse_plane), ("random", random_plane))
