"""Reference for the half buffers of rtow_mi355x.h ("half buffers") in numpy: the parity split of per-sample frames through
noise_ref.accumulate, n_h, the inputs of the two filter launches, denoise_ref.denoise with swapped guides, the combine, e_p and the frame
figures over the tree of noise_tree_ref.py in image order — every operation one IEEE operation in the header's order.  Also the designed
half states the GPU test imports."""
import numpy as np

import denoise_ref
import noise_ref
import noise_tree_ref

F32 = np.float32
NAN32 = np.uint32(0x7FC00000).view(F32)


def n_h(first_sample, n, h):
    """The number of absolute indices i in [first_sample, first_sample + n) with i & 1 == h; n a Python int or an integer array."""
    n = np.asarray(n, np.uint64)
    even = n // np.uint64(2) + (n & np.uint64(1) & np.uint64(~int(first_sample) & 1))
    out = n - even if h else even
    return int(out) if out.ndim == 0 else out


def n_h_brute(first_sample, n, h):
    return sum(1 for i in range(first_sample, first_sample + n) if i & 1 == h)


def split(frames, first_sample, counts=None):
    """frames[k]: the frame of the sample with the absolute index first_sample + k.  Returns per half (sum f32, S1, S2 f64): the in-order
    additions of the samples of parity h.  counts [rows, nx]: pixel p takes its first counts[p] samples only (an adaptive accumulation)."""
    frames = [np.asarray(f, F32) for f in frames]
    shape = frames[0].shape
    zero = (np.zeros(shape, F32), np.zeros(shape[:2]), np.zeros(shape[:2]), 0)
    out = []
    for h in range(2):
        mine = [(k, x) for k, x in enumerate(frames) if (first_sample + k) & 1 == h]
        if counts is None:
            total, s1, s2, _ = noise_ref.accumulate([x for _, x in mine]) if mine else zero
        else:  # pixel by count: the accumulation of the first m samples, picked where counts == m
            total, s1, s2, _ = zero
            for m in np.unique(counts):
                t, a, b, _ = noise_ref.accumulate([x for k, x in mine if k < m]) if any(k < m for k, _ in mine) else zero
                sel = counts == m
                total, s1, s2 = np.where(sel[..., None], t, total), np.where(sel, a, s1), np.where(sel, b, s2)
        out.append((total, s1, s2))
    return out


def figures_counted(s1, s2, n):
    """(Ybar, V) per pixel with a count per pixel (noise_ref.pixel_figures for every distinct count)."""
    n = np.broadcast_to(np.asarray(n, np.int64), np.shape(s1))
    ybar, v = np.zeros(np.shape(s1)), np.zeros(np.shape(s1))
    for k in np.unique(n):
        a, b = noise_ref.pixel_figures(s1, s2, int(k))
        ybar, v = np.where(n == k, a, ybar), np.where(n == k, b, v)
    return ybar, v


def read_half(total, s1, s2, nh):
    """rt_accum_read_halves: (sum / (float)max(n_h, 1), (float)sqrt(V_h))."""
    nh = np.broadcast_to(np.asarray(nh, np.int64), np.shape(s1))
    with np.errstate(all="ignore"):
        c = (np.asarray(total, F32) / np.maximum(nh, 1).astype(F32)[..., None]).astype(F32)
        sem = np.sqrt(figures_counted(s1, s2, nh)[1]).astype(F32)
    return c, sem


def inputs(total, s1, s2, nh):
    """(c_h, y_h, v_h) of one half: the guide is NaN where n_h < 2."""
    nh = np.broadcast_to(np.asarray(nh, np.int64), np.shape(s1))
    c, _ = read_half(total, s1, s2, nh)
    with np.errstate(all="ignore"):
        ybar, v = figures_counted(s1, s2, nh)
        y, v = ybar.astype(F32), v.astype(F32)
    return c, np.where(nh >= 2, y, NAN32), np.where(nh >= 2, v, NAN32)


def lum32(x):
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        return (F32(0.2126) * x[..., 0] + F32(0.7152) * x[..., 1]) + F32(0.0722) * x[..., 2]


def combine(f0, f1, n0, n1):
    """(out [rows, nx, 3] f32, e [rows, nx] f32)."""
    n0 = np.broadcast_to(np.asarray(n0, np.int64), f0.shape[:2])
    n1 = np.broadcast_to(np.asarray(n1, np.int64), f0.shape[:2])
    a0, a1 = n0.astype(F32), n1.astype(F32)
    with np.errstate(all="ignore"):
        out = (f0 * a0[..., None] + f1 * a1[..., None]) / (a0 + a1)[..., None]
        out = np.where((n1 == 0)[..., None], f0, np.where((n0 == 0)[..., None], f1, out))
        d = lum32(f0) - lum32(f1)
        e = (d * d) * ((a0 * a1) / ((a0 + a1) * (a0 + a1)))
        e = np.where((n0 == 0) | (n1 == 0), NAN32, e)
    assert out.dtype == F32 and e.dtype == F32
    return out, e


def residual(out, e):
    """(mean_luminance, residual_rms, residual_noise) over the pixels in image order on the tree of noise_tree_ref."""
    return noise_tree_ref.figures(lum32(out).astype(np.float64).reshape(-1), e.astype(np.float64).reshape(-1), 2)


def cross_filter(halves, first_sample, n, radius, patch, strength):
    """halves: [(sum, S1, S2)] x 2 in image order; n: done, or the per-pixel counts.  Returns dict(out, err, rgb8, residual, f, shares)."""
    nh = [n_h(first_sample, n, h) for h in range(2)]
    ins = [inputs(*halves[h], nh[h]) for h in range(2)]
    f, shares = [], []
    for h in range(2):
        o, s = denoise_ref.denoise(ins[h][0], ins[1 - h][1], ins[1 - h][2], radius, patch, strength)
        f.append(o), shares.append(s)
    out, e = combine(f[0], f[1], nh[0], nh[1])
    return dict(out=out, err=e, rgb8=denoise_ref.finalize_rgb8(out), residual=residual(out, e), f=f, shares=shares, inputs=ins)


# ---- designed half states: (halves, first_sample, done, counts or None), each half (sum, S1, S2) --------------------------------------
def state_from_inputs(c, y, v, nh):
    """A half (sum, S1, S2) whose inputs with n_h = nh (>= 2, a power of two here so that every step is exact or rounds once, knowingly)
    are close to (c, y, v): sum = c nh, S1 = y nh, S2 chosen so that V = v.  What the filter sees is defined by `inputs`, not by (c, y, v)."""
    c, y, v = np.asarray(c, F32), np.asarray(y, np.float64), np.asarray(v, np.float64)
    dn = float(nh)
    with np.errstate(all="ignore"):
        total = (c * F32(nh)).astype(F32)
        s1 = y * dn
        s2 = v * dn * (dn - 1.0) + s1 * s1 / dn
    return total, s1, s2


def kernel_halves(nx, rows, seeds=(11, 12), nh=8):
    """Two halves from denoise_ref.kernel_case with two seeds: the v = 0 block, a NaN and a +inf pixel — the non-finite ones in half 0
    only (half 1 gets finite values there)."""
    halves = []
    for h, seed in enumerate(seeds):
        c, y, v = denoise_ref.kernel_case(nx, rows, seed=seed)
        if h == 1:
            bad = ~np.isfinite(y) | ~np.isfinite(v)
            c, y, v = c.copy(), y.copy(), v.copy()
            c[bad], y[bad], v[bad] = [0.25, 0.5, 0.125], 0.4, 0.01
        halves.append(state_from_inputs(c, y, v, nh))
    return halves


def plain_halves(nx, rows, seeds=(7, 8), nh=8):
    return [state_from_inputs(*denoise_ref.synthetic(nx, rows, n=nh, seed=s)[1:], nh) for s in seeds]


def adaptive_counts(nx, rows, done=8):
    """Counts for an adaptive state beside done: pixels with n_p in {0, 1, 2, 3} (converged) spread over the frame, the others active."""
    cnt = np.full((rows, nx), done, np.uint32)
    conv = np.zeros((rows, nx), np.uint8)
    k = 0
    for j in range(rows):
        for i in range(nx):
            if j % 6 == 2 and i % 9 == 4:  # sparse: a pixel without a guide takes every patch that holds it out of the weights
                cnt[j, i], conv[j, i] = k % 4, 1
                k += 1
    return cnt, conv


def extremes_halves(nx=257, rows=256):
    """More than 256 partial sums, with the extremes of e behind pixel 65 536: smooth halves that differ by little, and two pixels in the
    last rows where they differ by much (one positive, one negative difference)."""
    yy, xx = np.mgrid[0:rows, 0:nx].astype(np.float64)
    base = 0.3 + 0.4 * (xx / nx) + 0.2 * (yy / rows)
    halves = []
    for h in range(2):
        y = base + (0.002 if h else -0.002) * np.sin(0.7 * xx + 1.3 * yy)
        c = np.stack([y, y * 0.5, y * 0.25], -1)
        v = np.full_like(y, 1e-4)
        if h == 0:
            c[rows - 1, 3], y[rows - 1, 3] = [40.0, 40.0, 40.0], 40.0
            c[rows - 2, nx - 5], y[rows - 2, nx - 5] = [1e-6, 1e-6, 1e-6], 1e-6
        halves.append(state_from_inputs(c.astype(F32), y, v, 8))
    return halves
