"""Reference for the sample buckets of rtow_mi355x.h ("sample buckets") in numpy: n_b, the split of per-sample frames by their absolute
index modulo M, the robust read-out — every operation one IEEE f32 operation in the header's order —, the frame figures over the tree of
noise_tree_ref.py in image order, and the filter on robust colours through denoise_ref.  Also the designed bucket states the GPU test
imports, and the two synthetic frames on which the estimator's gain and loss are shown."""
import numpy as np

import denoise_ref
import halves_ref
import noise_ref
import noise_tree_ref

F32 = np.float32
NAN32 = np.uint32(0x7FC00000).view(F32)
GINI, MEDIAN, TRIM = 0, 1, 2
BUCKETS_MAX = 16


def n_b(first_sample, n, M, b):
    """The number of absolute indices i in [first_sample, first_sample + n) with i % M == b; n a Python int or an integer array."""
    n = np.asarray(n, np.uint64)
    M64 = np.uint64(M)
    behind = np.uint64((b - first_sample % M) % M)
    out = n // M64 + (behind < n % M64).astype(np.uint64)
    return int(out) if out.ndim == 0 else out


def n_b_brute(first_sample, n, M, b):
    return sum(1 for i in range(first_sample, first_sample + n) if i % M == b)


def split(frames, first_sample, M, counts=None):
    """frames[k]: the frame of the sample with the absolute index first_sample + k.  Returns [M, rows, nx, 3] f32: per bucket the in-order
    additions of the samples with i % M == b.  counts [rows, nx]: pixel p takes its first counts[p] samples only (an adaptive accumulation)."""
    frames = [np.asarray(f, F32) for f in frames]
    out = np.zeros((M,) + frames[0].shape, F32)
    for k, x in enumerate(frames):
        b = (first_sample + k) % M
        with np.errstate(all="ignore"):
            added = (out[b] + x).astype(F32)
        out[b] = added if counts is None else np.where((k < np.asarray(counts))[..., None], added, out[b])
    return out


def robust(buckets, first_sample, n, mode=GINI, trim=0):
    """buckets [M, rows, nx, 3] f32 sums in image order; n: done, or the per-pixel counts [rows, nx].  Returns (out [rows, nx, 3] f32,
    t [rows, nx, 3] u8, dropped [rows, nx, 3] int): steps 1 to 4 of the header."""
    buckets = np.asarray(buckets, F32)
    M = buckets.shape[0]
    shape = buckets.shape[1:]
    with np.errstate(all="ignore"):
        nb = np.stack([np.broadcast_to(np.asarray(n_b(first_sample, n, M, b), np.int64), shape[:2]) for b in range(M)])[..., None]
        m = (buckets / np.maximum(nb, 1).astype(F32)).astype(F32)
        finite = (m - m) == 0
        keep = (nb > 0) & finite
        dropped = ((nb > 0) & ~finite).sum(0)
        K = keep.sum(0).astype(np.int64)
        x = np.sort(np.where(keep, m, F32(np.inf)), axis=0)  # the K kept means first, ascending
        tmax = np.maximum(K - 1, 0) // 2
        if mode == MEDIAN:
            t = tmax
        elif mode == TRIM:
            t = np.minimum(int(trim), tmax)
        else:
            s, w = np.zeros(shape, F32), np.zeros(shape, F32)
            for i in range(M):
                s = np.where(i < K, s + x[i], s).astype(F32)
                w = np.where(i < K, w + F32(i + 1) * x[i], w).astype(F32)
            fk = K.astype(F32)
            G = (F32(2.0) * w) / (fk * s) - ((K + 1).astype(F32) / fk)
            Gn = G * (fk / (K - 1).astype(F32))
            h = (Gn * fk) * F32(0.5)
            assert G.dtype == F32 and Gn.dtype == F32 and h.dtype == F32
            use = (K >= 2) & (s > 0) & (Gn > 0)
            cast = np.floor(np.minimum(np.where(use, h, F32(0)), F32(BUCKETS_MAX))).astype(np.int64)  # (uint32_t): toward zero; beyond every tmax: clamped below anyway
            t = np.where(use, np.minimum(cast, tmax), 0)
        a = np.zeros(shape, F32)
        for i in range(M):
            a = np.where((i >= t) & (i < K - t), a + x[i], a).astype(F32)
        out = np.where(K > 0, a / (K - 2 * t).astype(F32), NAN32).astype(F32)
        t = np.where(K > 0, t, 0)
    return out, t.astype(np.uint8), dropped


def plain(total, n):
    """c_p = sum_p / (float)max(n_p, 1)."""
    n = np.broadcast_to(np.asarray(n, np.int64), np.shape(total)[:2])
    with np.errstate(all="ignore"):
        return (np.asarray(total, F32) / np.maximum(n, 1).astype(F32)[..., None]).astype(F32)


def info(total, n, out, t, dropped):
    """RtRobustInfo as (mean_luminance_plain, mean_luminance_robust, energy_removed, trimmed_fraction, nonfinite_dropped)."""
    npix = np.float64(out.shape[0] * out.shape[1])
    with np.errstate(all="ignore"):
        lp = noise_tree_ref.tree_sum(halves_ref.lum32(plain(total, n)).astype(np.float64).reshape(-1)) / npix
        lr = noise_tree_ref.tree_sum(halves_ref.lum32(out).astype(np.float64).reshape(-1)) / npix
        removed = np.float64(1.0) - np.float64(lr) / np.float64(lp)
    if lp == 0.0 and lr == 0.0:
        removed = 0.0
    return float(lp), float(lr), float(removed), float(np.float64(int((t > 0).sum())) / (np.float64(3.0) * npix)), int(dropped.sum())


def read(buckets, total, first_sample, n, mode=GINI, trim=0):
    """rt_accum_read_robust: dict(out, trim, rgb8, info)."""
    out, t, dropped = robust(buckets, first_sample, n, mode, trim)
    return dict(out=out, trim=t, rgb8=denoise_ref.finalize_rgb8(out), info=info(total, n, out, t, dropped))


def means_readout(means, mode=GINI, trim=0):
    """The read-out of ONE pixel-channel from its bucket means (every bucket holding one sample): (out, t, dropped)."""
    b = np.asarray(means, F32).reshape(-1, 1, 1, 1) * np.ones((1, 1, 1, 3), F32)
    out, t, dropped = robust(b, 0, len(means), mode, trim)
    return out[0, 0, 0], int(t[0, 0, 0]), int(dropped[0, 0, 0])


def gini_h(means):
    """h = (Gn * K) * 0.5f of finite positive means, as step 3 forms it: what the cast to the trim sees."""
    x = np.sort(np.asarray(means, F32))
    K = len(x)
    s, w = F32(0), F32(0)
    for i in range(K):
        s = F32(s + x[i])
        w = F32(w + F32(F32(i + 1) * x[i]))
    fk = F32(K)
    G = F32(F32(F32(2.0) * w) / F32(fk * s) - F32(F32(K + 1) / fk))
    Gn = F32(G * F32(fk / F32(K - 1)))
    return F32(F32(Gn * fk) * F32(0.5))


def means_at_threshold(K, target, tries=40, seed=17):
    """(below, above): two lists of K means — K - 1 calm ones (equal at first, then drawn at random) and a larger one found by bisection
    over its bits and a walk over the neighbouring floats — with the largest h found below `target` and the smallest found at or above it.
    K = 16 reaches 1.0 and 2.0 exactly.  K = 5 cannot: 2w / (Ks) lies in [1, 2) there, so G = 2w / (Ks) - 1.2f moves in steps of 2^-23, and
    no such G gives (G * 1.25f * 5) * 0.5f = 1 or 2: the values on either side of each, a float or two away, are what there is."""
    target = F32(target)
    rng = np.random.default_rng(seed)
    below, above = None, None
    for k in range(tries):
        rest = [F32(1.0)] * (K - 1) if k == 0 else [F32(v) for v in 0.9 + 0.2 * rng.random(K - 1)]
        top = max(rest)
        lo, hi = F32(top), F32(top * 4096.0)
        assert gini_h(rest + [lo]) < target <= gini_h(rest + [hi])
        lo_b, hi_b = int(lo.view(np.uint32)), int(hi.view(np.uint32))
        while hi_b - lo_b > 1:
            mid = (lo_b + hi_b) // 2
            if gini_h(rest + [np.uint32(mid).view(F32)]) < target:
                lo_b = mid
            else:
                hi_b = mid
        for bits in range(lo_b - 8, hi_b + 9):  # (h is not monotone in the last bits: look around the flip)
            means = rest + [np.uint32(bits).view(F32)]
            h = gini_h(means)
            if h >= target and (above is None or h < gini_h(above)):
                above = means
            if h < target and (below is None or h > gini_h(below)):
                below = means
        if gini_h(above) == target and gini_h(below) == np.nextafter(target, F32(0)):
            break
    return below, above


# ---- designed states: (buckets [M, rows, nx, 3], total [rows, nx, 3], first_sample, done, counts or None, converged or None) ----------------
def designed_columns(K):
    """Lists of K bucket means, one pixel-channel each: the trim thresholds of GINI from both sides, one, two and (K + 1) / 2 firefly
    buckets, non-finite buckets, all non-finite, zero and negative sums, -0.0, ties."""
    cols = []
    for target in (1.0, 2.0):
        cols += list(means_at_threshold(K, target))
    calm = [F32(0.5 + 0.01 * i) for i in range(K)]
    for n_fire in (1, 2, (K + 1) // 2):
        cols.append(calm[:K - n_fire] + [F32(400.0 + 37.0 * i) for i in range(n_fire)])
    cols.append([np.nan] + calm[1:])
    cols.append([np.inf, -np.inf] + calm[2:])
    cols.append([np.nan, np.inf, -np.inf] + [F32(900.0)] + calm[4:])
    cols.append([np.nan, np.inf, -np.inf] + [np.nan] * (K - 3))
    cols.append([F32(0.0)] * K)
    cols.append([F32(-0.0)] * K)
    cols.append([F32(-0.0), F32(0.0)] * (K // 2) + [F32(0.0)] * (K % 2))
    cols.append([F32(-1.0 - i) for i in range(K)])
    cols.append([F32(-3.0)] + calm[1:])  # a negative mean among positive ones, s > 0
    cols.append([F32(-30.0)] + calm[1:])  # s < 0
    cols.append([F32(0.25)] * K)
    cols.append([F32(0.25)] * (K - 2) + [F32(8.0)] * 2)  # ties at both ends
    cols.append([F32(1e-42), F32(1e-45)] + calm[2:])  # denormals
    cols.append([F32(3e38), F32(3e38)] + calm[2:])  # s and w overflow
    return [[F32(v) for v in c] for c in cols]


def designed_state(K, nx, rows, first_sample, per_bucket=4, seed=3, counts=False):
    """M = K buckets that each hold `per_bucket` samples (a power of two: sum = mean * per_bucket and back are exact).  The designed columns
    go to the leading pixels of every channel, rolled by one pixel from channel to channel, in random bucket order; the rest is a calm
    frame with sparse fireflies.  counts: an adaptive state instead — per-pixel counts 0 .. M + 1 on the leading pixels of the second row
    on (converged), `done` = M * per_bucket on the others — with sums that are whatever they are: what n_b does to them is the point."""
    rng = np.random.default_rng(seed)
    M, done = K, K * per_bucket
    means = (0.3 + 0.5 * rng.random((M, rows, nx, 3))).astype(F32)
    fire = rng.random((M, rows, nx, 3)) < 0.02
    means = np.where(fire, means * F32(300.0), means).astype(F32)
    cols = designed_columns(K)
    assert len(cols) + 3 <= nx * rows
    flat = means.reshape(M, rows * nx, 3)
    for j, col in enumerate(cols):
        for c in range(3):
            flat[:, j + c, c] = np.asarray(col, F32)[rng.permutation(M)]
    with np.errstate(all="ignore"):
        buckets = (flat.reshape(M, rows, nx, 3) * F32(per_bucket)).astype(F32)
        total = np.zeros((rows, nx, 3), F32)
        for b in range(M):
            total = (total + buckets[b]).astype(F32)
    cnt = conv = None
    if counts:
        cnt, conv = np.full((rows, nx), done, np.uint32), np.zeros((rows, nx), np.uint8)
        for k in range(min(3 * (M + 2), nx * (rows - 1))):
            cnt[1 + k // nx, k % nx], conv[1 + k // nx, k % nx] = k % (M + 2), 1
    return buckets, total, first_sample, done, cnt, conv


def big_state(nx=257, rows=256, M=5, per_bucket=4):
    """More than 256 partial sums: a calm frame whose bucket means agree (t = 0), and behind the 65 536th pixel a pixel with one firefly
    bucket — its plain luminance is a hundred times the sum of all others, and it is the only trimmed one — and a pixel that is that bright
    in every bucket, so that the robust sum has its extreme there too: a final sum without its tail loses all three figures."""
    yy, xx = np.mgrid[0:rows, 0:nx].astype(np.float64)
    base = (0.3 + 0.4 * (xx / nx) + 0.2 * (yy / rows)).astype(F32)
    means = np.stack([np.stack([base * F32(1.0 + 0.01 * b), base * F32(0.5), base * F32(0.25 + 0.02 * b)], -1) for b in range(M)]).astype(F32)
    means[2, rows - 1, 3] = F32(5e7)
    means[:, rows - 1, 100] = F32(4e6)
    with np.errstate(all="ignore"):
        buckets = (means * F32(per_bucket)).astype(F32)
        total = np.zeros((rows, nx, 3), F32)
        for b in range(M):
            total = (total + buckets[b]).astype(F32)
    return buckets, total, 3, M * per_bucket, None, None


def denoise_robust(buckets, total, s1, s2, first_sample, n, radius, patch, strength, mode=GINI, trim=0):
    """rt_accum_denoise_robust: denoise_ref.denoise fed with the robust colours and the guide of the luminance moments (uniform: n = done)."""
    out, _, _ = robust(buckets, first_sample, n, mode, trim)
    with np.errstate(all="ignore"):
        ybar, v = noise_ref.pixel_figures(s1, s2, int(n))
        f, shares = denoise_ref.denoise(out, ybar.astype(F32), v.astype(F32), radius, patch, strength)
    return dict(out=f, rgb8=denoise_ref.finalize_rgb8(f), colours=out, shares=shares)


# ---- what the estimator is and is not ------------------------------------------------------------------------------------------------------
def firefly_frames(nx, rows, n, seed=7):
    """(truth, frames): sample k of every pixel is base * (U(0.5, 1.5) + 200 [u < 1/500]); per sample the uniform field is drawn first, then
    the firefly field.  The truth is base * 1.4."""
    rng = np.random.default_rng(seed)
    base = denoise_ref.truth_image(nx, rows).astype(np.float64)
    frames = []
    for _ in range(n):
        u = rng.uniform(0.5, 1.5, (rows, nx))
        f = rng.random((rows, nx)) < 1.0 / 500.0
        frames.append((base * (u + 200.0 * f)[..., None]).astype(F32))
    return (base * 1.4).astype(F32), frames


def synthetic_frames(nx, rows, n=16, seed=7):
    """(truth, frames) of denoise_ref.synthetic: the very samples it accumulates."""
    rng = np.random.default_rng(seed)
    truth = denoise_ref.truth_image(nx, rows)
    frames = []
    for _ in range(n):
        lit = rng.random((rows, nx)) < 0.25
        f = (4.0 * rng.uniform(0.5, 1.5, (rows, nx))) * lit
        frames.append((truth.astype(np.float64) * f[..., None]).astype(F32))
    return truth, frames


def estimator_errors(truth, frames, M):
    """dict(mean, gini, median: RMSE against the truth; info: of GINI; values: the frame's mean value plain, GINI, truth)."""
    n = len(frames)
    total = noise_ref.accumulate(frames)[0]
    buckets = split(frames, 0, M)
    g, m = read(buckets, total, 0, n, GINI), read(buckets, total, 0, n, MEDIAN)
    c = plain(total, n)
    return dict(mean=denoise_ref.rmse(c, truth), gini=denoise_ref.rmse(g["out"], truth), median=denoise_ref.rmse(m["out"], truth), info=g["info"],
                info_median=m["info"], values=(float(np.mean(c, dtype=np.float64)), float(np.mean(g["out"], dtype=np.float64)), float(np.mean(truth, dtype=np.float64))))


def designed_moments(total, done):
    """(S1, S2) f64 for a designed state: finite luminance moments whose Ybar follows the plain colour where that is finite (0.5 elsewhere)
    and whose V is (0.6 Ybar + 0.05)^2 — a guide under which neighbours of like luminance weight each other."""
    with np.errstate(all="ignore"):
        y = halves_ref.lum32(plain(total, done)).astype(np.float64)
    y = np.where(np.isfinite(y), np.clip(y, 0.0, 1e3), 0.5)
    _, s1, s2 = halves_ref.state_from_inputs(np.zeros(total.shape, F32), y, (0.6 * y + 0.05) ** 2, done)
    return s1, s2
