"""Reference for the accumulation of rtow_mi355x.h ("progressive accumulation") in numpy: the f32 sequential sum of per-sample frames,
the two f64 luminance moments and the figures derived from them, every operation one IEEE operation in the header's order."""
import numpy as np


def luminance(x):
    """Y = ((0.2126 (double)r + 0.7152 (double)g) + 0.0722 (double)b) of f32 samples [..., 3]."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return (0.2126 * x[..., 0] + 0.7152 * x[..., 1]) + 0.0722 * x[..., 2]


def accumulate(frames):
    """frames: a sequence of per-sample frames [rows, nx, 3] f32, in sample order.  Returns (sum f32 [rows, nx, 3], S1, S2 f64 [rows, nx], n):
    one addition per sample and accumulator, no pairwise summation."""
    frames = list(frames)
    shape = np.asarray(frames[0]).shape if frames else (0, 0, 3)
    total = np.zeros(shape, np.float32)
    s1 = np.zeros(shape[:2], np.float64)
    s2 = np.zeros(shape[:2], np.float64)
    for x in frames:
        x = np.asarray(x, dtype=np.float32)
        total = (total + x).astype(np.float32)
        y = luminance(x)
        s1 = s1 + y
        s2 = s2 + y * y
    return total, s1, s2, len(frames)


def pixel_figures(s1, s2, n):
    """(Ybar, V) per pixel: Ybar = S1 / n, V = max(0, (S2 - S1 S1 / n) / (n - 1)) / n; V = 0 where n < 2 and Ybar = 0 where n = 0."""
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    if n == 0:
        return np.zeros_like(s1), np.zeros_like(s1)
    dn = np.float64(n)
    ybar = s1 / dn
    if n < 2:
        return ybar, np.zeros_like(s1)
    with np.errstate(invalid="ignore"):
        q = (s2 - s1 * s1 / dn) / (dn - np.float64(1.0))
        v = np.where(q < 0.0, 0.0, q) / dn  # (a NaN stays one)
    return ybar, v


def sem(s1, s2, n):
    """out_sem = (float)sqrt(V)"""
    return np.sqrt(pixel_figures(s1, s2, n)[1]).astype(np.float32)


def frame_figures(s1, s2, n):
    """(mean_luminance, rms_sem, noise) of a frame, in f64."""
    ybar, v = pixel_figures(s1, s2, n)
    npix = np.float64(max(ybar.size, 1))
    mean = np.float64(np.sum(ybar)) / npix
    rms = np.sqrt(np.float64(np.sum(v)) / npix)
    if n < 2:
        noise = np.inf
    elif mean == 0.0:
        noise = 0.0 if rms == 0.0 else np.inf
    else:
        noise = rms / mean
    return float(mean), float(rms), float(noise)


def noise_of(frames):
    """The three frame figures of the accumulation of `frames`."""
    _, s1, s2, n = accumulate(frames)
    return frame_figures(s1, s2, n)
