"""Reference for the channel moments and the colour-guided filter of rtow_mi355x.h ("channel moments and the colour-guided filter") in
numpy: the f64 replay of the moments over per-sample frames, and the filter in f32 with every operation one IEEE operation in the header's
order (numpy's element-wise operators never fuse), so that the kernels can be held to both bit for bit.  Also the synthetic frames the tests
feed it.  denoise_ref and noise_ref are imported and left as they are."""
import numpy as np

import denoise_ref
import noise_ref

F32 = np.float32
KERNEL_CASE_STRENGTH = denoise_ref.KERNEL_CASE_STRENGTH


# ---- the moments ----------------------------------------------------------------------------------------------------------------------
def accumulate_channels(frames, counts=None):
    """frames: per-sample frames [rows, nx, 3] f32 in sample order.  counts (u32 [rows, nx], optional): pixel p takes its first counts[p]
    frames only (an adaptive accumulation).  Returns (S1, S2) f64 [rows, nx, 3]: S1_c += (double)x_c, S2_c += (double)x_c * (double)x_c."""
    frames = [np.asarray(x, dtype=F32) for x in frames]
    s1 = np.zeros(frames[0].shape, np.float64)
    s2 = np.zeros(frames[0].shape, np.float64)
    for k, x in enumerate(frames):
        d = x.astype(np.float64)
        with np.errstate(all="ignore"):
            n1, n2 = s1 + d, s2 + d * d
        if counts is None:
            s1, s2 = n1, n2
        else:
            take = (k < np.asarray(counts))[..., None]
            s1, s2 = np.where(take, n1, s1), np.where(take, n2, s2)
    return s1, s2


def channel_variance(s1, s2, n):
    """V_c = max(0, (S2_c - S1_c S1_c / n) / (n - 1)) / n in f64, 0 where n < 2; n a number or a u32 array [rows, nx]."""
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    n = np.asarray(n, np.uint32)
    n = np.broadcast_to(n[..., None] if n.ndim else n, s1.shape)
    dn = n.astype(np.float64)
    with np.errstate(all="ignore"):
        q = (s2 - s1 * s1 / dn) / (dn - np.float64(1.0))
        v = np.where(q < 0.0, 0.0, q) / dn  # (a NaN stays one)
    return np.where(n >= 2, v, 0.0)


def channel_sem(s1, s2, n):
    """out_sem_rgb = (float)sqrt(V_c)"""
    with np.errstate(invalid="ignore"):
        return np.sqrt(channel_variance(s1, s2, n)).astype(F32)


# ---- the filter -----------------------------------------------------------------------------------------------------------------------
def denoise(c, var, radius, patch, strength):
    """c, var [rows, nx, 3] in image order -> (out [rows, nx, 3] f32, shares) as denoise_ref.denoise returns them: denoise_ref.nlm with
    the three guide planes (c_ch, var_ch), so a term is (d_r + d_g) + d_b and the divisor 3 (2F + 1)^2."""
    c, var = np.asarray(c, F32), np.asarray(var, F32)
    return denoise_ref.nlm(c, [(c[..., ch], var[..., ch]) for ch in range(3)], radius, patch, strength)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
def luminance709(rgb):
    rgb = np.asarray(rgb, np.float64)
    return (0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1]) + 0.0722 * rgb[..., 2]


BAND_COLOURS = ((1.0, 0.2, 0.0), (0.0, 0.5, 0.0), (0.2, 0.3, 1.0), (1.0, 1.0, 1.0))  # each scaled to Rec. 709 luminance BAND_LUMINANCE
BAND_LUMINANCE = 0.4


def truth_bands(nx, rows):
    """denoise_ref.truth_image with its right half replaced by four horizontal bands of equal Rec. 709 luminance 0.4: orange, green, blue
    and grey.  Returns (truth f32 [rows, nx, 3], the mask [rows, nx] of the banded half)."""
    img = denoise_ref.truth_image(nx, rows).astype(np.float64)
    half = np.zeros((rows, nx), bool)
    half[:, nx // 2:] = True
    for k, col in enumerate(BAND_COLOURS):
        col = np.asarray(col, np.float64)
        col = col * (BAND_LUMINANCE / luminance709(col))
        img[rows * k // 4:rows * (k + 1) // 4, nx // 2:] = col
    return img.astype(F32), half


def synthetic_channels(nx, rows, n=16, seed=7, truth=None):
    """denoise_ref.synthetic — the same random numbers in the same order, so the same frames — with the channel variances as well:
    (truth, c, y, v, var_rgb); `truth` None: denoise_ref.truth_image."""
    rng = np.random.default_rng(seed)
    truth = denoise_ref.truth_image(nx, rows) if truth is None else np.asarray(truth, F32)
    frames = []
    for _ in range(n):
        lit = rng.random((rows, nx)) < 0.25
        f = (4.0 * rng.uniform(0.5, 1.5, (rows, nx))) * lit
        frames.append((truth.astype(np.float64) * f[..., None]).astype(F32))
    total, s1, s2, _ = noise_ref.accumulate(frames)
    ybar, var = noise_ref.pixel_figures(s1, s2, n)
    var_rgb = channel_variance(*accumulate_channels(frames), n)
    return truth, (total / F32(n)).astype(F32), ybar.astype(F32), var.astype(F32), var_rgb.astype(F32)


def kernel_case(nx, rows, seed=11):
    """(c, var_rgb) that exercises the kernel, after denoise_ref.kernel_case: the synthetic frame; a block of pixels with all three v = 0, its
    left half one constant colour, its right half the noisy values it had; one pixel with v = 0 in one channel only; and, where the frame is
    large enough, one NaN and one +inf pixel away from each other."""
    _, c, _, _, var = synthetic_channels(nx, rows, seed=seed)
    c, var = c.copy(), var.copy()
    if nx >= 8 and rows >= 6:
        y0, x0, h, w = rows // 2, nx // 8, max(rows // 4, 2), max(nx // 4, 4)
        var[y0:y0 + h, x0:x0 + w] = 0
        c[y0:y0 + h, x0:x0 + w // 2] = [0.5, 0.25, 0.75]
        var[2, nx // 2, 1] = 0
        c[1, nx - 2], var[1, nx - 2] = np.nan, np.nan
        c[rows - 2, 1] = np.inf
        var[rows - 2, 1] = np.nan  # (the moments of an infinite sample: S2 - S1 S1 / n = inf - inf)
    return c, var
