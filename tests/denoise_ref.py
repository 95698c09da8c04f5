"""Reference for the filter of rtow_mi355x.h ("denoising") in numpy: f32 throughout, every operation one IEEE operation in the header's
order (numpy's element-wise operators never fuse), so that the kernel can be held to it bit for bit.  Also the synthetic noisy frame the
tests feed it."""
import numpy as np

import noise_ref

F32 = np.float32
EPS = F32(1e-10)
KERNEL_CASE_STRENGTH = 0.45  # at which kernel_case(37, 21) with (R 5, F 1) has >= 10 % of its pairs in each weight class (test_denoise_host.py)


def nlm(colours, guides, radius, patch, strength):
    """The body both filters share.  colours [rows, nx, 3]; guides: a list of (mean, variance) planes [rows, nx], all in image order.  A
    term of the patch distance is the left-to-right sum of the planes' d, the divisor len(guides) (2F + 1)^2.  Returns (out [rows, nx, 3]
    f32, shares), shares = the fractions of the in-image (p, q) pairs with w == 0, 0 < w < 1 and w == 1."""
    c, guides = np.asarray(colours, F32), [(np.asarray(g, F32), np.asarray(v, F32)) for g, v in guides]
    (rows, nx), R, F, k = c.shape[:2], int(radius), int(patch), F32(strength)
    k2, cnt = F32(k * k), F32(len(guides) * (2 * F + 1) * (2 * F + 1))
    (ys, xs), (ye, xe) = np.mgrid[0:rows, 0:nx], np.mgrid[-F:rows + F, -F:nx + F]

    def at(a, yy, xx):
        return a[np.clip(yy, 0, rows - 1), np.clip(xx, 0, nx - 1)]

    def d(g, v, ay, ax, by, bx):  # one plane's d between the pixels a and b, each clamped on its own
        diff, va, vb = at(g, ay, ax) - at(g, by, bx), at(v, ay, ax), at(v, by, bx)
        return (diff * diff - (va + np.where(vb < va, vb, va))) / (EPS + k2 * (va + vb))

    den, num, n = np.zeros((rows, nx), F32), np.zeros((rows, nx, 3), F32), [0, 0, 0]
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < nx)
                terms = [d(g, v, ye, xe, ye + dy, xe + dx) for g, v in guides]  # at every x = p + o, once: all (p, o) with this x share it
                e = sum(terms[1:], terms[0])  # (left to right; one plane: d itself.  q outside the image: masked out below)
                S = np.zeros((rows, nx), F32)
                for oy in range(F + F + 1):
                    row = np.zeros((rows, nx), F32)
                    for ox in range(F + F + 1):
                        row = row + e[oy:oy + rows, ox:ox + nx]
                    S = S + row
                D = S / cnt
                u = F32(1) - F32(0.25) * np.where(D < 0, F32(0), D)  # max(D, 0), but a NaN stays
                u = np.where(u > 0, u, F32(0))  # a NaN becomes 0
                w = (u * u) * (u * u)
                use = inside & (u != 0)
                den = np.where(use, den + w, den)
                num = np.where(use[..., None], num + w[..., None] * at(c, qy, qx), num)
                n = [a + int((inside & cls).sum()) for a, cls in zip(n, (w == 0, (w > 0) & (w < 1), w == 1))]
        out = np.where((den == 0)[..., None], c, num / den[..., None])
    assert out.dtype == F32 and den.dtype == F32 and num.dtype == F32
    return out, tuple(x / max(sum(n), 1) for x in n)


def denoise(c, y, v, radius, patch, strength):
    """c [rows, nx, 3], y, v [rows, nx] in image order -> (out, shares) of nlm with the one guide plane (y, v)."""
    return nlm(c, [(y, v)], radius, patch, strength)


def truth_image(nx, rows):
    """A piecewise-smooth frame with edges: a horizontal gradient, a bright disc, a dark coloured bar and a vertical step."""
    yy, xx = np.mgrid[0:rows, 0:nx].astype(np.float64)
    fx, fy = xx / max(nx - 1, 1), yy / max(rows - 1, 1)
    img = np.stack([0.2 + 0.5 * fx, 0.3 + 0.3 * fy, 0.5 - 0.3 * fx], axis=-1)
    disc = (fx - 0.3) ** 2 * (nx / max(rows, 1)) ** 2 + (fy - 0.55) ** 2 < 0.08
    img[disc] = [1.2, 1.0, 0.6]
    bar = (fy > 0.15) & (fy < 0.3) & (fx > 0.5)
    img[bar] = [0.05, 0.1, 0.3]
    img[(fx > 0.8)] *= 0.4
    return img.astype(F32)


def synthetic(nx, rows, n=16, seed=7):
    """(truth, c, y, v): n heavy-tailed samples per pixel — 0 with probability 3/4, else 4 x truth x U(0.5, 1.5) — accumulated as
    tests/noise_ref.py accumulates them; c = sum / (float)n, y = (float)Ybar, v = (float)V."""
    rng = np.random.default_rng(seed)
    truth = truth_image(nx, rows)
    frames = []
    for _ in range(n):
        lit = rng.random((rows, nx)) < 0.25
        f = (4.0 * rng.uniform(0.5, 1.5, (rows, nx))) * lit
        frames.append((truth.astype(np.float64) * f[..., None]).astype(F32))
    total, s1, s2, _ = noise_ref.accumulate(frames)
    ybar, var = noise_ref.pixel_figures(s1, s2, n)
    return truth, (total / F32(n)).astype(F32), ybar.astype(F32), var.astype(F32)


def rmse(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt(np.mean(d * d)))


def finalize_rgb8(img):
    """k_finalize's quantisation and flip of an f32 image [rows, nx, 3]: sqrt, * 255.99f, saturating u8 (NaN and negatives: 0), row 0 on top."""
    with np.errstate(all="ignore"):
        g = (np.sqrt(np.asarray(img, F32)) * F32(255.99)).astype(F32)
        ok = (g == g) & (g > 0)
        q = np.where(ok, np.minimum(g, F32(255)), F32(0)).astype(np.uint32).astype(np.uint8)  # (toward zero; 255 and beyond: 255)
    return q[::-1].copy()


def kernel_case(nx, rows, seed=11):
    """(c, y, v) that exercises the kernel: the synthetic frame, a block of pixels with v = 0 (its left half one constant value, its right
    half the noisy values it had) and, where the frame is large enough, one NaN and one +inf pixel away from each other."""
    _, c, y, v = synthetic(nx, rows, seed=seed)
    c, y, v = c.copy(), y.copy(), v.copy()
    if nx >= 8 and rows >= 6:
        y0, x0, h, w = rows // 2, nx // 8, max(rows // 4, 2), max(nx // 4, 4)
        v[y0:y0 + h, x0:x0 + w] = 0
        c[y0:y0 + h, x0:x0 + w // 2] = [0.5, 0.25, 0.75]
        y[y0:y0 + h, x0:x0 + w // 2] = 0.5
        c[1, nx - 2], y[1, nx - 2] = np.nan, np.nan
        v[1, nx - 2] = np.nan
        c[rows - 2, 1], y[rows - 2, 1] = np.inf, np.inf
        v[rows - 2, 1] = np.nan  # (the moments of an infinite sample: S2 - S1 S1 / n = inf - inf)
    return c, y, v
