"""Reference for adaptive sampling (rtow_mi355x.h "adaptive sampling") in numpy f64: the stopping criterion, and a replay of an
accumulation step by step over single-sample frames (the method of noise_ref.py), which predicts per pixel the sample count, the sums,
the sem and the frame figures.  Every operation is one IEEE operation in the header's order."""
import numpy as np

import noise_ref


def pixel_figures(s1, s2, cnt):
    """(Ybar, V) per pixel with the pixel's own n: noise_ref.pixel_figures, n an array."""
    s1, s2, cnt = np.asarray(s1, np.float64), np.asarray(s2, np.float64), np.asarray(cnt)
    ybar, v = np.zeros_like(s1), np.zeros_like(s1)
    for n in np.unique(cnt):
        m = cnt == n
        y, w = noise_ref.pixel_figures(s1[m], s2[m], int(n))
        ybar[m], v[m] = y, w
    return ybar, v


def converged(s1, s2, n, tolerance, luminance_floor, min_samples):
    """The criterion on the moments of n samples: n >= min_samples && V <= thr * thr, thr = tolerance * max(Ybar, floor),
    max(a, b) = a > b ? a : b.  A NaN compares false."""
    ybar, v = noise_ref.pixel_figures(s1, s2, int(n))
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(ybar > np.float64(luminance_floor), ybar, np.float64(luminance_floor))
        thr = np.float64(tolerance) * m
        return (int(n) >= int(min_samples)) & (v <= thr * thr)


class Replay:
    """An accumulation that begins at sample 0 over the single-sample frames x[s] ([rows, nx, 3] f32).  uniform(n) is rt_accum_add,
    adaptive(n, ...) is rt_accum_add_adaptive: the decision on what every active pixel holds, sticky, then n samples for the rest."""

    def __init__(self, frames):
        self.x = [np.asarray(f, np.float32) for f in frames]
        shape = self.x[0].shape
        self.total = np.zeros(shape, np.float32)
        self.s1, self.s2 = np.zeros(shape[:2], np.float64), np.zeros(shape[:2], np.float64)
        self.cnt = np.zeros(shape[:2], np.uint32)
        self.conv = np.zeros(shape[:2], bool)
        self.issued = 0
        self.stopped_at = np.zeros(shape[:2], np.int64) - 1  # the n_p at which a pixel converged, -1 while active
        self.traced = []  # primary rays of every add

    def _add(self, n, active):
        for s in range(self.issued, self.issued + n):
            x = self.x[s]
            y = noise_ref.luminance(x)
            self.total = np.where(active[..., None], (self.total + x).astype(np.float32), self.total)
            self.s1 = np.where(active, self.s1 + y, self.s1)
            self.s2 = np.where(active, self.s2 + y * y, self.s2)
        self.cnt = np.where(active, self.cnt + np.uint32(n), self.cnt).astype(np.uint32)
        self.issued += n
        self.traced.append(int(active.sum()) * n)

    def uniform(self, n):
        assert not self.conv.any()
        self._add(n, np.ones_like(self.conv))

    def adaptive(self, n, tolerance, luminance_floor, min_samples):
        now = ~self.conv & converged(self.s1, self.s2, self.issued, tolerance, luminance_floor, min_samples)
        self.stopped_at[now] = self.issued
        self.conv |= now
        self._add(n, ~self.conv)
        return int((~self.conv).sum())  # n_active

    def set_moments(self, pixel, s1, s2):
        self.s1.reshape(-1)[pixel], self.s2.reshape(-1)[pixel] = s1, s2

    def image(self):
        """sum / (float)n_p (n_p 0: / 1)"""
        return (self.total / np.maximum(self.cnt, 1).astype(np.float32)[..., None]).astype(np.float32)

    def sem(self):
        return np.sqrt(pixel_figures(self.s1, self.s2, self.cnt)[1]).astype(np.float32)

    def frame_figures(self):
        """(mean_luminance, rms_sem, noise) in f64; noise is +inf where any n_p < 2."""
        ybar, v = pixel_figures(self.s1, self.s2, self.cnt)
        npix = np.float64(max(ybar.size, 1))
        mean = np.float64(np.sum(ybar)) / npix
        rms = np.sqrt(np.float64(np.sum(v)) / npix)
        if (self.cnt < 2).any():
            noise = np.inf
        elif mean == 0.0:
            noise = 0.0 if rms == 0.0 else np.inf
        else:
            noise = rms / mean
        return float(mean), float(rms), float(noise)

    def info(self):
        """(n_active, n_samples, spp_min, spp_max)"""
        return int((~self.conv).sum()), int(self.cnt.astype(np.uint64).sum()), int(self.cnt.min()), int(self.cnt.max())


def relative_error(frames, n, luminance_floor):
    """sqrt(V) / max(Ybar, floor) per pixel after the first n frames: what a tolerance is compared with."""
    _, s1, s2, _ = noise_ref.accumulate(frames[:n])
    ybar, v = noise_ref.pixel_figures(s1, s2, n)
    return np.sqrt(v) / np.where(ybar > luminance_floor, ybar, luminance_floor)
