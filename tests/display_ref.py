"""Reference for the display transform of rtow_mi355x.h ("display transform") in numpy: f32 step by step, every operation one IEEE
operation in the header's order (numpy's element-wise operators never fuse), f64 only where the header says so — the logarithms and their
sum on the tree of tests/noise_tree_ref.py, the quotient behind e, the power of the sRGB transfer.  The kernels are held to it bit for bit;
under the sRGB transfer outside the AMBIGUOUS values, whose level differs between y (1 - EPS) and y (1 + EPS).

EPS = RT_DISPLAY_SRGB_EPS = 2^-20 is derived, not fitted.  p = (float)pow((double)t, 1 / 2.4): a conforming f64 pow is within 16 ulp
(glibc's and the device library's within 1), so two implementations round to the same f32 except within 2^-48 of a rounding boundary
and then differ by one ulp of p, at most 2^-23 p.  1.055f * p rounds once more on either side: the two products differ by at most
2 ulp of the product a.  a - 0.055f rounds once more on either side (half an ulp of y <= half an ulp of a each): the two y differ by at
most 3 ulp(a) <= 3 * 2^-23 a, and a / y = 1.055 p / (1.055 p - 0.055) <= 2.36 on t > 0.0031308 (p >= 0.0905).  3 * 2.36 * 2^-23 =
14.2 * 2^-24 < 2^-20."""
import numpy as np

import noise_tree_ref

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -20
MANUAL, KEY, PERCENTILE = 0, 1, 2
CLAMP, REINHARD, ACES = 0, 1, 2
GAMMA2, SRGB = 0, 1
NONE, BAYER8 = 0, 1
BINS = 2048
FLT_MAX = np.finfo(F32).max


def bayer(x, y):
    """B(x, y) of the header, on integers or integer arrays."""
    b = 0
    for k in range(3):
        b = b | ((((x ^ y) >> k) & 1) << (2 * (2 - k) + 1)) | (((y >> k) & 1) << (2 * (2 - k)))
    return b


def luminance(rgb):
    rgb = np.asarray(rgb, F32)
    with np.errstate(all="ignore"):
        return (F32(0.2126) * rgb[..., 0] + F32(0.7152) * rgb[..., 1]) + F32(0.0722) * rgb[..., 2]


def histogram(rgb):
    """(hist [2048] of bits(Y) >> 20 over the lit pixels, n_lit)."""
    return histogram_y(luminance(rgb))


def histogram_y(y):
    """The same of given f32 luminances."""
    y = np.asarray(y, F32).reshape(-1)
    lit = np.isfinite(y) & (y > 0)
    bins = np.ascontiguousarray(y[lit]).view(np.uint32) >> 20
    return np.bincount(bins, minlength=BINS).astype(np.uint64), int(lit.sum())


def rank_of(q, n_lit):
    """max(1, ceil(q * n_lit)) with q an f32: the f64 product is exact below 2^29 pixels."""
    return max(1, int(np.ceil(F64(F32(q)) * F64(n_lit))))


def bin_mid(b):
    return np.array([(int(b) << 20) | 0x80000], np.uint32).view(F32)[0]


def _exposure(value, denominator):
    with np.errstate(all="ignore"):
        e = F32(F64(F32(value)) / F64(denominator))
    return e if np.isfinite(e) and e > 0 else F32(1)


def statistics(rgb, d):
    """{exposure, percentile_luminance, log_average, n_lit} of the image [rows, nx, 3] in the call's row order under the display d."""
    out = {"exposure": F32(d.exposure_value), "percentile_luminance": F32(0), "log_average": 0.0, "n_lit": 0}
    if d.exposure_mode == MANUAL:
        return out
    y = luminance(rgb).reshape(-1)
    lit = np.isfinite(y) & (y > 0)
    n_lit = out["n_lit"] = int(lit.sum())
    out["exposure"] = F32(1)
    if n_lit == 0:
        return out
    if d.exposure_mode == KEY:
        with np.errstate(all="ignore"):
            logs = np.where(lit, np.log(np.where(lit, y, F32(1)).astype(F64)), 0.0)
        s = noise_tree_ref.tree_sum(logs)  # 256 consecutive pixels of the image per partial sum, then the final workgroup
        out["log_average"] = float(np.exp(F64(s) / F64(n_lit)))
        out["exposure"] = _exposure(d.exposure_value, out["log_average"])
    else:
        hist, _ = histogram(rgb)
        b = int(np.searchsorted(np.cumsum(hist), rank_of(d.percentile, n_lit), side="left"))
        out["percentile_luminance"] = bin_mid(b)
        out["exposure"] = _exposure(d.exposure_value, out["percentile_luminance"])
    return out


def _levels(y, dither, offset, dtype):
    """The quantisation of y (any float type, computed in `dtype`): g, then k_finalize's rule."""
    with np.errstate(all="ignore"):
        y = np.asarray(y, dtype)
        g = y * dtype(255.0) + offset.astype(dtype) if dither else y * dtype(F32(255.99))
        ok = (g == g) & (g > 0)
        return np.where(ok, np.minimum(g, dtype(255)), dtype(0)).astype(np.uint32)


def display(rgb, d, e=None):
    """(rgb8 [rows, nx, 3] with row 0 on top, info) of the image [rows, nx, 3] in the call's row order.  A given e bypasses the
    statistics (info then carries no n_lit).  info["ambiguous"]: under the sRGB transfer the mask [rows, nx, 3], laid out as rgb8, of the
    values whose level differs between y (1 - EPS) and y (1 + EPS), with info["level_lo"] and info["level_hi"] the two levels; else None."""
    c = np.ascontiguousarray(rgb, F32)
    rows, nx = c.shape[:2]
    info = statistics(c, d) if e is None else {"exposure": F32(e)}
    e = F32(info["exposure"])
    lj, i = np.mgrid[0:rows, 0:nx]
    r = rows - 1 - lj  # the row of out_rgb8
    dither = d.dither == BAYER8
    offset = ((bayer(i & 7, r & 7).astype(F32) + F32(0.5)) / F32(64.0))[..., None]
    with np.errstate(all="ignore"):
        fin = np.isfinite(c)
        bad = ~fin.all(axis=-1)
        x = e * c
        x = np.where(x > 0, x, F32(0))
        t = x
        if d.curve == REINHARD:
            L = luminance(x)
            w = F32(d.white)
            s = (F32(1) + L / (w * w)) / (F32(1) + L)
            t = x * s[..., None]
        elif d.curve == ACES:
            xa = np.where(x < F32(65536.0), x, F32(65536.0))
            t = (xa * (F32(2.51) * xa + F32(0.03))) / (xa * (F32(2.43) * xa + F32(0.59)) + F32(0.14))
        t = np.where(bad[..., None], x, t).astype(F32)  # a pixel with a non-finite channel: its finite channels as under CLAMP
        ambiguous = None
        if d.transfer == SRGB:
            p = np.power(t.astype(F64), 1.0 / 2.4).astype(F32)
            linear = t <= F32(0.0031308)
            y = np.where(linear, F32(12.92) * t, F32(1.055) * p - F32(0.055)).astype(F32)
            lo, hi = _levels(y.astype(F64) * (1 - EPS), dither, offset, F64), _levels(y.astype(F64) * (1 + EPS), dither, offset, F64)
            ambiguous = (lo != hi) & ~linear & fin
            info["level_lo"], info["level_hi"] = lo[::-1].astype(np.uint8), hi[::-1].astype(np.uint8)
        else:
            y = np.sqrt(t)
        assert y.dtype == F32 and t.dtype == F32 and x.dtype == F32
        u = _levels(y, dither, offset, F32)
        u = np.where(fin, u, np.where(c > 0, 255, 0)).astype(np.uint32)  # +inf: 255; -inf and a NaN: 0
    info["n_non_finite"] = int(bad.sum())
    info["n_saturated"] = int((u == 255).sum())
    info["ambiguous"] = None if ambiguous is None else ambiguous[::-1].copy()
    return u.astype(np.uint8)[::-1].copy(), info


def make(exposure=1.0, auto=MANUAL, percentile=0.99, curve=CLAMP, white=np.inf, transfer=GAMMA2, dither=NONE):
    """A display for this module alone (the attributes of an RtDisplay), for the tests that need no library."""
    import types
    return types.SimpleNamespace(exposure_mode=auto, exposure_value=F32(exposure), percentile=F32(percentile), curve=curve, white=F32(white),
                                 transfer=transfer, dither=dither, reserved=0)


# ---- the planes of the tests ----------------------------------------------------------------------------------------------------------------
FRAMES = ((1, 1), (7, 5), (64, 3), (300, 220))  # 7 and 5: the Bayer tile wraps unaligned; 66 000 pixels: 258 partial sums, a final loop of two trips
AMBIGUOUS_CAP = 0.005                           # of the values of a plane under the sRGB transfer; the reference's own share is about 1e-4


def designed_pixels():
    """[N, 3] f32: the values where the pixel stage can go wrong.  The quantisation bits of tests/designed_states.py (either side of every
    step of the reference quantisation, the special bit patterns, NaN and the infinities among them) rolled through the three channels;
    negative values; and every subset of the channels non-finite — one, two or three of them, as NaN, +inf and -inf, mixed too."""
    import designed_states
    bits = designed_states.quantisation_bits()
    m = bits.size
    j = np.arange(m)
    quant = np.stack([bits[(j + ch * (m // 3)) % m] for ch in range(3)], axis=1).view(F32)
    rng = np.random.default_rng(17)
    neg = -np.exp2(rng.uniform(-20, 20, (32, 3))).astype(F32)
    neg[::2, 1] = -neg[::2, 1]  # (half of them mixed with a positive channel)
    bad = []
    for subset in range(1, 8):
        for kind in ((np.nan,) * 3, (np.inf,) * 3, (-np.inf,) * 3, (np.nan, np.inf, -np.inf), (-np.inf, np.nan, np.inf)):
            bad.append([kind[ch] if subset >> ch & 1 else (0.04, 0.5, 3.0)[ch] for ch in range(3)])
    return np.concatenate([quant, neg, np.array(bad, F32)]).astype(F32)


def designed_plane(nx, rows):
    """[rows, nx, 3]: designed_pixels laid over the frame pixel by pixel, starting at an offset that differs per frame so that the small
    frames see different ones; repeated where the frame is larger."""
    px = designed_pixels()
    idx = (np.arange(nx * rows) + 131 * nx + 7 * rows) % len(px)
    return px[idx].reshape(rows, nx, 3).copy()


def statistics_plane(nx, rows, seed=9):
    """The random plane of the statistics tests: log-uniform luminances over 2^-12 .. 2^12, a tenth of the pixels black, a few negative,
    NaN and infinite ones, and — where the frame has more than 65 536 pixels — the extreme values (2^-100, 2^100) behind the 65 536th, where
    only the second trip of the final workgroup's loop sees them."""
    rng = np.random.default_rng([seed, nx, rows])
    img = np.exp2(rng.uniform(-12, 12, (rows * nx, 1)) + rng.uniform(-1, 1, (rows * nx, 3))).astype(F32)
    n = rows * nx
    img[rng.random(n) < 0.1] = 0
    if n >= 16:
        img[rng.integers(0, n, 3)] = -1.0
        img[rng.integers(0, n, 1), 1] = np.nan
        img[rng.integers(0, n, 1), 2] = np.inf
    if n > 65536:
        img[65536 + 100] = F32(2.0 ** -100)
        img[65536 + 300] = F32(2.0 ** 100)
    return img.reshape(rows, nx, 3)
def log_uniform_plane(nx, rows, seed=5, lo=-20.0, hi=20.0):
    """[rows, nx, 3] f32, 2^U(lo, hi) per value from a seeded generator."""
    rng = np.random.default_rng([seed, nx, rows])
    return np.exp2(rng.uniform(lo, hi, (rows, nx, 3))).astype(F32)


def srgb_boundary_values(dither_offset=None):
    """The f32 inputs t whose sRGB value y lies 8 EPS (relative) below and above every level boundary k / 255.99, k = 1 .. 255 (no
    dither): unambiguous by construction — and close enough that a transfer wrong in its sixth digit shows."""
    k = np.arange(1, 256, dtype=F64)
    out = []
    for side in (1 - 8 * EPS, 1 + 8 * EPS):
        y = k / F64(F32(255.99)) * side
        t = np.where(y <= 12.92 * 0.0031308, y / 12.92, ((y + 0.055) / 1.055) ** 2.4)
        out.append(t)
    return np.concatenate(out).astype(F32)
