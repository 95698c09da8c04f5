"""Reference for the multi-scale filter of rtow_mi355x.h ("multi-scale denoising") in numpy, on top of denoise_ref.nlm: f32 throughout,
every operation one IEEE operation in the header's order (numpy's element-wise operators never fuse), so that the kernels of
csrc/rt_multiscale.h can be held to it bit for bit.  denoise_ref is imported and left as it is."""
import numpy as np

import denoise_ref

F32 = np.float32
MAX_LEVELS = 4
W_NEAR, W_SIDE, W_FAR = F32(0.5625), F32(0.1875), F32(0.0625)  # 2x bilinear interpolation at pixel centres: 9/16, 3/16, 1/16


def level_size(nx, rows, level):
    """(nx_l, rows_l): a side halves, rounded up, per level; a side of 1 stays 1."""
    for _ in range(level):
        nx, rows = (nx + 1) // 2, (rows + 1) // 2
    return nx, rows


def down(a, variance=False):
    """D of the header on a plane [rows, nx] or an image [rows, nx, channels]: the four taps of a coarse pixel, those outside the image
    +0, summed as (t00 + t10) + (t01 + t11) and scaled by 1 / k (a mean) or 1 / (k k) (the variance of a mean of k independent means),
    k = the taps inside the image: 1, 2 or 4."""
    a = np.asarray(a, F32)
    rows, nx = a.shape[:2]
    nx1, rows1 = level_size(nx, rows, 1)
    t = np.zeros((2 * rows1, 2 * nx1) + a.shape[2:], F32)
    t[:rows, :nx] = a
    with np.errstate(all="ignore"):
        total = (t[0::2, 0::2] + t[0::2, 1::2]) + (t[1::2, 0::2] + t[1::2, 1::2])
        ky = 1 + (2 * np.arange(rows1) + 1 < rows)
        kx = 1 + (2 * np.arange(nx1) + 1 < nx)
        k = (ky[:, None] * kx[None, :]).astype(F32)
        scale = F32(1) / (k * k if variance else k)  # 1, 0.5, 0.25 or 0.0625: exact
        out = total * (scale if a.ndim == 2 else scale[..., None])
    assert out.dtype == F32
    return out


def residual(o_coarse, f_fine):
    """e = o_{s+1} - D(F_s) per channel at level s + 1; an e that is not finite is +0."""
    with np.errstate(all="ignore"):
        e = np.asarray(o_coarse, F32) - down(f_fine)
    return np.where(np.isfinite(e), e, F32(0)).astype(F32)


def up_add(f_fine, e):
    """o_s = F_s + U(e): U the 2x bilinear interpolation at pixel centres, clamped at the border, summed as
    (0.5625 e(X, Y) + 0.1875 e(X', Y)) + (0.1875 e(X, Y') + 0.0625 e(X', Y'))."""
    f_fine, e = np.asarray(f_fine, F32), np.asarray(e, F32)
    rows, nx = f_fine.shape[:2]
    rows1, nx1 = e.shape[:2]
    y, x = np.mgrid[0:rows, 0:nx]
    X, Y = x >> 1, y >> 1
    X2 = np.clip(X + np.where(x & 1, 1, -1), 0, nx1 - 1)
    Y2 = np.clip(Y + np.where(y & 1, 1, -1), 0, rows1 - 1)
    with np.errstate(all="ignore"):
        u = (W_NEAR * e[Y, X] + W_SIDE * e[Y, X2]) + (W_SIDE * e[Y2, X] + W_FAR * e[Y2, X2])
        out = f_fine + u
    assert out.dtype == F32
    return out


def multiscale(c, guides, radius, patch, strength, levels):
    """c [rows, nx, 3]; guides: a list of (mean, variance) planes [rows, nx] as denoise_ref.nlm takes them, all in image order.  Returns
    (o_0 [rows, nx, 3] f32, per level s a dict of the filter's inputs `c` and `guides`, its output `F`, its weight `shares` and `o`)."""
    assert 1 <= levels <= MAX_LEVELS
    c = np.asarray(c, F32)
    guides = [(np.asarray(m, F32), np.asarray(v, F32)) for m, v in guides]
    lv = []
    for s in range(levels):
        if s:
            c, guides = down(c), [(down(m), down(v, variance=True)) for m, v in guides]
        f, shares = denoise_ref.nlm(c, guides, radius, patch, strength)
        lv.append({"c": c, "guides": guides, "F": f, "shares": shares})
    lv[-1]["o"] = lv[-1]["F"]
    for s in range(levels - 2, -1, -1):
        lv[s]["e"] = residual(lv[s + 1]["o"], lv[s]["F"])
        lv[s]["o"] = up_add(lv[s]["F"], lv[s]["e"])
    return lv[0]["o"], lv


def luminance(c, y, v, radius, patch, strength, levels):
    """The luminance guide: one plane (y, v)."""
    return multiscale(c, [(y, v)], radius, patch, strength, levels)


def channels(c, var, radius, patch, strength, levels):
    """The channels guide: three planes (c_ch, var_ch); the guide means are the colours."""
    c, var = np.asarray(c, F32), np.asarray(var, F32)
    return multiscale(c, [(c[..., ch], var[..., ch]) for ch in range(3)], radius, patch, strength, levels)
