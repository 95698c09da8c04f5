"""The frame figures of an accumulation (rtow_mi355x.h "Frame figures") by the very tree the kernels add over, so that they can be held
bit for bit: block_sum_256 of csrc/rt_kernels.h, k_noise_partials<COUNTS>, k_noise_final<COUNTS>, and the integer sums of
adaptive_block_sums, k_adaptive_decide and k_adaptive_info (csrc/rt_adaptive.h), restated in numpy f64 — every addition one IEEE
addition, in the kernel's order.

  lanes   : lane 0's chain of `for off = 32, 16, .., 1: a += __shfl_down(a, off)` is a halving tree over the 64 lanes of a wave
            (after the step `off`, lane i < off holds lane i + lane i + off of the step before);
  waves   : ((w0 + w1) + w2) + w3;
  partials: workgroup b takes the pixels 256 b .. 256 b + 255 of the accumulation's LOCAL pixel order (tests/frame_cases.py
            local_of_pixel), slots past npix add 0.0;
  final   : thread t of ONE workgroup adds the partials t, t + 256, ... onto 0.0 in index order, then lanes and waves as above.

`tail=False` drops every trip of the final loop but the first (what a kernel without the loop would compute): tests use it to show
that a frame reaches the tail.  exact_figures and figure_bound are the independent check: math.fsum and the analytic error bound of
the tree."""
import math

import numpy as np

import frame_cases

U = 2.0 ** -53  # the relative error of one f64 operation rounded to nearest


def local_index(nx, rows, tpr, tile_pixels):
    """[rows, nx] -> the local index of every pixel (frame_cases.local_of_pixel, pixel by pixel)."""
    out = np.empty((rows, nx), np.int64)
    for lj in range(rows):
        for i in range(nx):
            out[lj, i] = frame_cases.local_of_pixel(nx, tpr, tile_pixels, i, lj)
    return out


def to_local(plane, loc):
    """An image-order plane [rows, nx] as the flat array the accumulation keeps."""
    flat = np.empty(loc.size, np.asarray(plane).dtype)
    flat[loc.reshape(-1)] = np.asarray(plane).reshape(-1)
    return flat


def block_sum_256(a):
    """a [nb, 256] f64 -> [nb]: lanes by the halving tree, the four waves in wave order."""
    w = np.asarray(a, np.float64).reshape(-1, 4, 64)
    with np.errstate(all="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            w = w[..., :off] + w[..., off:2 * off]
        w = w[..., 0]
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def partials(local):
    """k_noise_partials: one sum per workgroup of 256 consecutive local pixels."""
    nb = max(-(-local.size // 256), 1)
    padded = np.zeros(nb * 256, np.float64)
    padded[:local.size] = local
    return block_sum_256(padded.reshape(nb, 256))


def final_sum(parts, tail=True):
    """k_noise_final's sum: thread t adds parts[t], parts[t + 256], ... onto 0.0, then block_sum_256 over the 256 threads."""
    trips = -(-parts.size // 256) if tail else min(1, parts.size)
    acc = np.zeros(256, np.float64)
    with np.errstate(all="ignore"):
        for k in range(trips):
            chunk = np.zeros(256, np.float64)
            part = parts[256 * k:256 * k + 256]
            chunk[:part.size] = part
            acc = np.where(np.arange(256) < part.size, acc + chunk, acc)
        return float(block_sum_256(acc.reshape(1, 256))[0])


def tree_sum(local, tail=True):
    return final_sum(partials(np.asarray(local, np.float64)), tail)


def figures(ybar_local, v_local, spp_min, tail=True):
    """(mean_luminance, rms_sem, noise) as k_noise_final<false> / k_noise_final<true> write them; spp_min: `done` of a uniform accumulation."""
    npix = np.float64(ybar_local.size)
    with np.errstate(all="ignore"):
        mean = np.float64(tree_sum(ybar_local, tail)) / npix
        rms = np.sqrt(np.float64(tree_sum(v_local, tail)) / npix)
        noise = rms / mean
    if mean == 0.0:
        noise = 0.0 if rms == 0.0 else np.inf
    if spp_min < 2:
        noise = np.inf
    return float(mean), float(rms), float(noise)


def adaptive_info(cnt_local, conv_local, tail=True):
    """(n_active, n_samples, spp_min, spp_max) through k_adaptive_decide's partial sums and k_adaptive_info: 64-bit sums, u32 min and max,
    slots past npix contributing (0, 0, 0xFFFFFFFF, 0)."""
    cnt = [int(c) for c in np.asarray(cnt_local).reshape(-1)]
    act = [0 if c else 1 for c in np.asarray(conv_local).reshape(-1)]
    M = (1 << 64) - 1
    parts = []
    for b in range(max(-(-len(cnt) // 256), 1)):
        c, a = cnt[256 * b:256 * b + 256], act[256 * b:256 * b + 256]
        parts.append((sum(a) & M, sum(c) & M, min(c + [0xFFFFFFFF]), max(c + [0])))
    threads = []
    for t in range(256):
        mine = parts[t::256] if tail else parts[t:t + 1]
        threads.append((sum(p[0] for p in mine) & M, sum(p[1] for p in mine) & M, min([p[2] for p in mine] + [0xFFFFFFFF]),
                        max([p[3] for p in mine] + [0])))
    return (sum(p[0] for p in threads) & M, sum(p[1] for p in threads) & M, min(p[2] for p in threads), max(p[3] for p in threads))


# ---- the independent check ------------------------------------------------------------------------------------------------------------
def chain_length(npix):
    """The most additions any term passes through on its way into the frame's sum: 6 lane steps and 3 wave steps in its workgroup, one
    addition per trip of the final loop (the first, onto 0.0, is exact and counted all the same), then 6 + 3 again."""
    nb = -(-npix // 256)
    return 9 + -(-nb // 256) + 9


def figure_bound(npix):
    """Relative error bounds (mean_luminance, rms_sem, noise) of the tree against the exact figures, for finite non-negative terms.
    A sum of non-negative terms in which no term passes through more than d roundings is within (1 + U)^d - 1 of the exact sum,
    relatively.  mean = sum / npix adds one rounding: (1 + U)^(d + 1) - 1 <= (d + 2) U for d U << 1.  rms = sqrt(sum / npix): the square
    root halves the relative error of its argument and adds a rounding of its own, ((d + 1) / 2 + 1) U <= (d + 2) U.  noise = rms / mean:
    both errors and the division's.  exact_figures itself carries up to 2 U (fsum's rounding and its own division or square root), which
    the bounds include."""
    d = chain_length(npix)
    one = (d + 2 + 2) * U
    return one, one, 2 * one + U


def exact_figures(ybar, v):
    """(mean_luminance, rms_sem, noise) from the exactly rounded sums (math.fsum) of finite Ybar and finite non-negative V."""
    ybar, v = np.asarray(ybar, np.float64).reshape(-1), np.asarray(v, np.float64).reshape(-1)
    assert np.isfinite(ybar).all() and np.isfinite(v).all() and (v >= 0).all()
    mean = math.fsum(ybar) / ybar.size
    rms = math.sqrt(math.fsum(v) / v.size)
    return mean, rms, (rms / mean if mean else np.inf)


def abs_mean(ybar):
    """(sum |Ybar|) / npix: what the bound on mean_luminance is relative to where Ybar has both signs — a sum in which no term passes
    through more than d roundings is within ((1 + U)^d - 1) sum |x| of the exact sum."""
    ybar = np.asarray(ybar, np.float64).reshape(-1)
    return math.fsum(np.abs(ybar)) / ybar.size
