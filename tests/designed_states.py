"""Designed accumulation states (numpy only, no GPU): the planes of an RtAccumState in image order whose values sit where a read-out
kernel can go wrong — on either side of every 8-bit quantisation step, at sample counts (float)n rounds, at moments whose variance
cancels to either side of zero, at pixels exactly on the adaptive threshold.  rt_accum_import puts them in front of the kernels with no
ray traced (tests/test_designed_states.py); tests/test_designed_states_host.py shows on the references alone that every state has the
property it is built for.

A state is the dict of accum_state_ref.make_state plus "where": class name -> boolean mask [rows, nx] of the pixels that carry the class,
so that a failing assertion can say which class failed.  Everything else is filled with finite, positive, varied values from a seeded
generator.  A pixel whose sum is not finite gets non-finite moments as well, as a non-finite sample would leave it ("non_finite_sum")."""
import numpy as np

import accum_state_ref
import adaptive_ref
import denoise_ref
import noise_ref

F32 = np.float32
UNIFORM_DONE = (1, 2, 3, 7, 16777217, 4294967295)  # 1: the quantisation plane undivided; 2: q == 0 throughout; 3, 7: quotients that round;
LARGE_DONE = (16777217, 4294967295)                # the last two: (float)n rounds to 16777216 and to 2^32
COUNTS_DONE = (2, 24, 16777217, 4294967295)
MAGNITUDES = (1e-160, 1e-30, 1.0, 1e30, 1e150)
NORMAL_MAGNITUDES = (1e-30, 1.0, 1e30)             # where neither y y nor S1 S1 leaves the normal range for any n
PER_MAGNITUDE = 96
SEQUENTIAL_UP_TO = 1000                            # constant samples are accumulated one by one up to this n, as n y and n (y y) beyond
SPECIAL_BITS = (0x00000000, 0x80000000, 0x00000001, 0x00800000, 0x3F7FFFFF, 0x3F800000, 0x3F800001, 0x7F7FFFFF, 0x7F800000, 0xFF800000,
                0xBF800000, 0x7FC01234)            # +0, -0, the smallest denormal, FLT_MIN, 1 - ulp, 1, 1 + ulp, FLT_MAX, +inf, -inf, -1, a NaN
TIE_BITS = tuple(int(np.float32(k * 2.0 ** -118).view(np.uint32)) for k in (5, 9, 13))  # / 2^32: 2.5, 4.5 and 6.5 denormal steps, ties
NAN64 = np.array([0x7FF8DEADBEEF0001], np.uint64).view(np.float64)[0]


def f32_of_bits(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(F32)


def quantise(c):
    """denoise_ref.finalize_rgb8 on a flat array of f32 values (one row: the flip moves nothing)."""
    c = np.ascontiguousarray(c, dtype=F32).reshape(1, -1, 1)
    return denoise_ref.finalize_rgb8(np.repeat(c, 3, axis=2))[0, :, 0]


def quantisation_boundaries():
    """bits[k - 1], k = 1 .. 255: the smallest positive f32 whose reference quantisation is >= k, by bisection over the float's bits
    (the quantisation is monotone over the positive floats, which order as their bits do)."""
    k = np.arange(1, 256)
    lo, hi = np.zeros(255, np.uint32), np.full(255, 0x3F800000, np.uint32)  # q(+0) = 0 < k, q(1.0) = 255 >= k
    while (hi - lo > 1).any():
        mid = ((lo.astype(np.uint64) + hi) // 2).astype(np.uint32)
        ge = quantise(f32_of_bits(mid)) >= k
        hi, lo = np.where(ge, mid, hi), np.where(ge, lo, mid)
    return hi


def quantisation_bits():
    """The values of the Quantisation class as bits: the predecessor of every boundary and the boundary, k = 1 .. 255, then SPECIAL_BITS,
    then TIE_BITS — sums whose quotient by (float)(2^32 - 1) = 2^32 is a tie between two denormals and rounds to the even one, while the
    quotient by 2^32 - 1 in f64, a little larger, rounds up: where a division by the unrounded count shows at this n."""
    b = quantisation_boundaries()
    return np.concatenate([np.stack([b - 1, b], axis=1).reshape(-1), np.array(SPECIAL_BITS + TIE_BITS, np.uint32)])


def sum_plane(npix, rng):
    """([npix, 3] f32, the number of leading pixels that carry the Quantisation class).  Pixel j carries the values j, j + m/3 and
    j + 2m/3 (mod m) of quantisation_bits: its three channels hold different boundaries, and every value passes through every channel."""
    bits = quantisation_bits()
    m = bits.size
    assert npix >= m, (npix, m)
    plane = rng.uniform(0.05, 4.0, (npix, 3)).astype(F32)
    j = np.arange(m)
    for ch in range(3):
        plane.view(np.uint32)[:m, ch] = bits[(j + ch * (m // 3)) % m]
    return plane, m


def constant_samples(y, n, rng):
    """(S1, S2) of n[k] samples that are all y[k]: one addition per sample up to SEQUENTIAL_UP_TO, n y and n (y y) beyond; S2 is then
    moved by -2 .. 2 ulps (a fifth of the pixels stay as accumulated), as the roundings of samples that differ in their last bits would
    scatter it.  S1 = n y and S2 = n y^2 up to rounding, so that S2 - S1 S1 / n cancels to a few ulps on either side of zero — as
    accumulated it is exactly 0 in a third to a half of the pixels."""
    y, n = np.asarray(y, np.float64), np.asarray(n, np.uint64)
    ulps = np.where(n == 2, 0, rng.integers(-2, 3, y.shape))  # (two equal samples cancel exactly: n = 2 stays the class q == 0)
    s1, s2 = np.zeros_like(y), np.zeros_like(y)
    with np.errstate(all="ignore"):
        yy = y * y
        small = n <= SEQUENTIAL_UP_TO
        for s in range(int(n[small].max()) if small.any() else 0):
            m = small & (s < n)
            s1, s2 = np.where(m, s1 + y, s1), np.where(m, s2 + yy, s2)
        dn = n.astype(np.float64)
        s1, s2 = np.where(small, s1, dn * y), np.where(small, s2, dn * yy)
        for k in (1, 2):
            s2 = np.where(ulps >= k, np.nextafter(s2, np.inf), np.where(ulps <= -k, np.nextafter(s2, -np.inf), s2))
    return s1, s2


NON_FINITE_MOMENTS = ((NAN64, 1.0), (1.0, NAN64), (np.inf, 1.0), (1.0, np.inf), (-np.inf, np.inf), (np.inf, np.inf), (NAN64, np.inf), (-1.0, -np.inf))


def moments_plane(n, rng):
    """(S1, S2 [npix] f64, {class: slice}) for the per-pixel sample counts n [npix]: the Moments class in the leading pixels, in this
    order — constant samples at each of MAGNITUDES ("const 1e-30", ...), S2 = 0 with S1 != 0, both zero, a negative S1, non-finite
    slots — then varied finite positive moments with a comfortable variance."""
    n = np.asarray(n, np.uint64)
    npix = n.size
    dn = n.astype(np.float64)
    y = rng.uniform(0.05, 1.0, npix)
    s = y * rng.uniform(0.02, 0.5, npix)
    with np.errstate(all="ignore"):
        s1, s2 = dn * y, dn * (y * y + s * s)
        where, at = {}, 0
        for mag in MAGNITUDES:
            sl = slice(at, at + PER_MAGNITUDE)
            s1[sl], s2[sl] = constant_samples(mag * rng.uniform(0.5, 2.0, PER_MAGNITUDE), n[sl], rng)
            where["const %g" % mag], at = sl, at + PER_MAGNITUDE
        sl = slice(at, at + 8)
        s1[sl], s2[sl], where["s2 zero"], at = dn[sl] * rng.uniform(0.1, 1.0, 8), 0.0, sl, at + 8
        sl = slice(at, at + 4)
        s1[sl], s2[sl], where["zero"], at = 0.0, 0.0, sl, at + 4
        sl = slice(at, at + 8)
        yn = rng.uniform(0.1, 1.0, 8)
        s1[sl], s2[sl], where["negative s1"], at = -dn[sl] * yn, dn[sl] * (yn * yn) * 1.1, sl, at + 8
        sl = slice(at, at + len(NON_FINITE_MOMENTS))
        s1[sl], s2[sl] = [a for a, _ in NON_FINITE_MOMENTS], [b for _, b in NON_FINITE_MOMENTS]
        where["non-finite"], at = sl, at + len(NON_FINITE_MOMENTS)
    assert at <= npix
    return s1, s2, where


def counts_plane(npix, done, rng):
    """(counts u32, converged u8 [npix]): about half of the pixels converged, their counts spread over [2, done] with 2, done and — where
    done allows — 2^31 - 1, 2^31 and 2^31 + 1 among them; the active ones hold `done`.  done < 2: every pixel active."""
    if done < 2:
        return np.full(npix, done, np.uint32), np.zeros(npix, np.uint8)
    conv = rng.random(npix) < 0.5
    conv[:8] = [True, False] * 4
    cnt = np.minimum(2 + np.floor(rng.random(npix) * (done - 1)).astype(np.uint64), done)
    pins = [2, done] + [c for c in (2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1) if c <= done]
    cnt[np.flatnonzero(conv)[:len(pins)]] = pins
    return np.where(conv, cnt, done).astype(np.uint32), conv.astype(np.uint8)


def _masks(where, nx, rows):
    out = {}
    for name, sl in where.items():
        m = np.zeros(nx * rows, bool)
        m[sl] = True
        out[name] = m.reshape(rows, nx)
    return out


def state(nx, rows, done, seed=1, counts=False, channels=False, frame_id=0):
    """The designed state of the read-out tests: the Quantisation class in the sums, the Moments class in the luminance moments and —
    `channels` — per channel, each channel's classes rolled to other pixels; `counts`: an adaptive state, the Counts class."""
    rng = np.random.default_rng([seed, nx, rows, done % 65521, int(counts), int(channels)])
    npix = nx * rows
    total, m = sum_plane(npix, rng)
    cnt, conv = counts_plane(npix, done, rng) if counts else (np.full(npix, done, np.uint32), None)
    s1, s2, where = moments_plane(cnt, rng)
    where = _masks(dict(where, quant=slice(0, m)), nx, rows)
    chm = None
    if channels:
        chm = np.zeros((npix, 6), np.float64)
        for ch in range(3):
            shift = 97 * (ch + 1)
            c1, c2, w = moments_plane(np.roll(cnt, -shift), rng)
            chm[:, 2 * ch], chm[:, 2 * ch + 1] = np.roll(c1, shift), np.roll(c2, shift)
            where.update({"ch%d %s" % (ch, k): np.roll(v.reshape(-1), shift).reshape(rows, nx) for k, v in _masks(w, nx, rows).items()})
    bad = ~np.isfinite(total).all(axis=1)  # a non-finite sum: the moments a non-finite sample leaves
    s1[bad], s2[bad] = NAN64, NAN64
    if channels:
        chm[bad] = NAN64
    bad = bad.reshape(rows, nx)
    where = {k: v & ~bad if k != "quant" else v for k, v in where.items()}
    where["non_finite_sum"] = bad
    st = accum_state_ref.make_state(nx, rows, 0, done, frame_id, total.reshape(rows, nx, 3), s1.reshape(rows, nx), s2.reshape(rows, nx),
                                    counts=cnt.reshape(rows, nx) if counts else None, converged=conv.reshape(rows, nx) if counts else None,
                                    channel_moments=chm.reshape(rows, nx, 6) if channels else None)
    st["where"] = where
    return st


# ---- what the read-out must return (the references, on a state) ---------------------------------------------------------------------------
def pixel_counts(st):
    """n_p per pixel: the counts of an adaptive state, `done` of a uniform one."""
    return st["counts"] if st["planes"] & accum_state_ref.COUNTS else np.full((st["rows"], st["nx"]), st["done"], np.uint32)


def image(st):
    """rt_accum_read's f32 image: sum / (float)n_p, n_p 0: / 1 — one f32 division by the count ROUNDED TO f32."""
    with np.errstate(all="ignore"):
        return (st["sum"] / np.maximum(pixel_counts(st), 1).astype(F32)[..., None]).astype(F32)


def image_f64(st):
    """What a kernel that divided in f64 and rounded once would return: not the header's value."""
    with np.errstate(all="ignore"):
        return (st["sum"].astype(np.float64) / np.maximum(pixel_counts(st), 1).astype(np.float64)[..., None]).astype(F32)


def figures(st):
    """(Ybar, V) f64 [rows, nx] with the pixel's own n_p."""
    with np.errstate(all="ignore"):
        return adaptive_ref.pixel_figures(st["moments"][..., 0], st["moments"][..., 1], pixel_counts(st))


def variance_before_clamp(s1, s2, n):
    """q = (S2 - S1 S1 / n) / (n - 1) before max(0, q): what the clamp of pixel_noise sees."""
    dn = np.asarray(n, np.float64)
    with np.errstate(all="ignore"):
        return (np.asarray(s2, np.float64) - np.asarray(s1, np.float64) * np.asarray(s1, np.float64) / dn) / (dn - 1.0)


def denoise_inputs(st):
    """(c, y, v) f32 as k_denoise_inputs<COUNTS> forms them: c = sum / (float)n_p, y = (float)Ybar, v = (float)V; a pixel with n_p < 2:
    c = sum / (float)max(n_p, 1), y = v = NaN."""
    ybar, v = figures(st)
    n = pixel_counts(st)
    with np.errstate(all="ignore"):
        c = (st["sum"] / np.maximum(n, 1).astype(F32)[..., None]).astype(F32)
        return c, np.where(n < 2, F32(np.nan), ybar.astype(F32)), np.where(n < 2, F32(np.nan), v.astype(F32))


def channel_inputs(st):
    """(c, var) f32 [rows, nx, 3] as k_denoise_inputs_channels forms them: c = sum / (float)n_p (no / 1), var = (float)V_ch."""
    import denoise_channels_ref
    n = pixel_counts(st)
    with np.errstate(all="ignore"):
        c = (st["sum"] / n.astype(F32)[..., None]).astype(F32)
        return c, denoise_channels_ref.channel_variance(*channel_planes(st), n).astype(F32)


def finite_copy(st, limit=None, seed=11):
    """`st` with the luminance moments of every pixel whose Ybar or V is not finite — and, with `limit`, whose moments exceed it in
    magnitude — replaced by varied finite positive ones for the pixel's own n_p: the state whose three frame figures are numbers.
    Every other class stays where it is."""
    rng = np.random.default_rng([seed, st["nx"], st["rows"]])
    ybar, v = figures(st)
    bad = ~np.isfinite(ybar) | ~np.isfinite(v) | ~np.isfinite(st["moments"]).all(axis=-1)
    if limit is not None:
        bad |= (np.abs(st["moments"]) > limit).any(axis=-1)
    dn = pixel_counts(st).astype(np.float64)
    y = rng.uniform(0.05, 1.0, dn.shape)
    s = y * rng.uniform(0.02, 0.5, dn.shape)
    mom = st["moments"].copy()
    mom[..., 0], mom[..., 1] = np.where(bad, dn * y, mom[..., 0]), np.where(bad, dn * (y * y + s * s), mom[..., 1])
    out = dict(st, moments=mom)
    out["where"] = dict(st["where"], replaced=bad)
    return out


def channel_planes(st):
    """(S1, S2) [rows, nx, 3] of the channel moments."""
    return st["channel_moments"][..., 0::2], st["channel_moments"][..., 1::2]


# ---- the Thresholds class -------------------------------------------------------------------------------------------------------------
def threshold_of(s1, n, tolerance, floor):
    """thr * thr of adaptive_ref.converged for the moments' Ybar."""
    with np.errstate(all="ignore"):
        ybar = np.asarray(s1, np.float64) / np.float64(n)
        m = np.where(ybar > np.float64(floor), ybar, np.float64(floor))
        thr = np.float64(tolerance) * m
        return thr * thr


def _v(s1, s2, n):
    return noise_ref.pixel_figures(s1, s2, n)[1]


def s2_hitting(s1, n, wanted, reach=96):
    """(S2, found): S2 within `reach` ulps of the algebraic solution for which noise_ref.pixel_figures returns exactly the V `wanted`.
    S2 - S1 S1 / n cancels, so one ulp of S2 moves V by many of its own ulps and only some (S1, wanted) can be hit: `found` says which."""
    s1, wanted = np.asarray(s1, np.float64), np.asarray(wanted, np.float64)
    start = wanted * n * (n - 1.0) + s1 * s1 / n
    out, found = start.copy(), np.zeros(s1.shape, bool)
    for direction in (np.inf, -np.inf):
        cand = start.copy()
        for _ in range(reach):
            hit = (_v(s1, cand, n) == wanted) & ~found
            out, found = np.where(hit, cand, out), found | hit
            cand = np.nextafter(cand, direction)
    return out, found


def s2_straddling(s1, n, t):
    """(lo, hi), hi the successor of lo: the two neighbouring S2 with V(lo) <= t < V(hi) — as close to the threshold from either side
    as the moments allow."""
    s1, t = np.asarray(s1, np.float64), np.asarray(t, np.float64)
    lo = t * n * (n - 1.0) + s1 * s1 / n
    for _ in range(4096):
        above = _v(s1, lo, n) > t
        if not above.any():
            break
        lo = np.where(above, np.nextafter(lo, -np.inf), lo)
    for _ in range(4096):
        nxt = np.nextafter(lo, np.inf)
        more = _v(s1, nxt, n) <= t
        if not more.any():
            break
        lo = np.where(more, nxt, lo)
    hi = np.nextafter(lo, np.inf)
    assert (_v(s1, lo, n) <= t).all() and (_v(s1, hi, n) > t).all()
    return lo, hi


THRESHOLD_CLASSES = ("v exact", "v succ", "v pred", "floor branch exact", "floor branch succ", "floor branch pred", "straddle le", "straddle gt",
                     "ybar floor le", "ybar floor gt", "ybar above floor le", "ybar above floor gt", "ybar below floor le", "ybar below floor gt",
                     "negative ybar le", "negative ybar gt", "nan v", "v zero", "imported converged")


def threshold_state(nx, rows, n, tolerance, floor, seed=3, frame_id=0):
    """An adaptive state of `n` issued samples for the decision of rt_accum_add_adaptive(tolerance, floor): every class of
    THRESHOLD_CLASSES in the leading pixels, the rest active with a V between a quarter and four times its threshold.
      v exact / succ / pred      : Ybar above the floor, V exactly thr thr, its successor, its predecessor
      floor branch ...           : the same with S1 = 0 (Ybar = 0: the floor decides thr), where every V can be hit
      straddle le / gt           : neighbouring S2 whose V lie on either side of thr thr
      ybar (above / below) floor : Ybar == floor and one ulp either side, each with the two straddling S2
      negative ybar, nan v, v zero (exact cancellation, and a negative q the clamp lifts to 0)
      imported converged         : flagged converged with fewer samples and moments that fail the criterion, or NaN"""
    rng = np.random.default_rng([seed, nx, rows, n])
    npix, dn = nx * rows, float(n)
    y = rng.uniform(0.05, 1.0, npix)
    s1 = dn * y
    t = threshold_of(s1, n, tolerance, floor)
    s2 = t * rng.uniform(0.25, 4.0, npix) * dn * (dn - 1.0) + s1 * s1 / dn
    cnt, conv = np.full(npix, n, np.uint32), np.zeros(npix, np.uint8)
    where, at = {}, 0

    def put(name, a, b):
        nonlocal at
        k = len(a)
        s1[at:at + k], s2[at:at + k] = a, b
        where[name], at = slice(at, at + k), at + k

    pool = dn * rng.uniform(0.05, 1.0, 40000)  # Ybar well above the floor
    tp = threshold_of(pool, n, tolerance, floor)
    for name, wanted in (("v exact", tp), ("v succ", np.nextafter(tp, np.inf)), ("v pred", np.nextafter(tp, -np.inf))):
        b, found = s2_hitting(pool, n, wanted)
        pick = np.flatnonzero(found)[:8]
        assert pick.size >= 4, (name, pick.size)
        put(name, pool[pick], b[pick])
    t0 = threshold_of(np.zeros(1), n, tolerance, floor)
    for name, wanted in (("floor branch exact", t0), ("floor branch succ", np.nextafter(t0, np.inf)), ("floor branch pred", np.nextafter(t0, -np.inf))):
        b, found = s2_hitting(np.zeros(1), n, wanted)
        assert found.all(), name
        put(name, np.zeros(1), b)
    a = dn * rng.uniform(0.05, 1.0, 24)
    lo, hi = s2_straddling(a, n, threshold_of(a, n, tolerance, floor))
    put("straddle le", a, lo), put("straddle gt", a, hi)
    for name, yb in (("ybar floor", floor), ("ybar above floor", np.nextafter(floor, np.inf)), ("ybar below floor", np.nextafter(floor, -np.inf)),
                     ("negative ybar", -0.3)):
        a = np.array([dn * yb])
        lo, hi = s2_straddling(a, n, threshold_of(a, n, tolerance, floor))
        put(name + " le", a, lo), put(name + " gt", a, hi)
    put("nan v", [NAN64, 1.0, np.inf, 2.0], [1.0, NAN64, np.inf, np.inf])
    a = dn * rng.uniform(0.05, 1.0, 4)
    put("v zero", a, [a[0] * a[0] / dn, a[1] * a[1] / dn, 0.0, a[3] * a[3] / dn * 0.5])
    k = 16
    a = dn * rng.uniform(0.05, 1.0, k)
    b = a * a  # S2 = S1^2: V of the order of Ybar^2, far above any threshold
    a[:2], b[:2] = NAN64, NAN64
    cnt[at:at + k], conv[at:at + k] = rng.integers(2, n + 1, k), 1
    cnt[at], cnt[at + 1] = 2, n
    put("imported converged", a, b)
    total = rng.uniform(0.05, 4.0, (npix, 3)).astype(F32)
    st = accum_state_ref.make_state(nx, rows, 0, n, frame_id, total.reshape(rows, nx, 3), s1.reshape(rows, nx), s2.reshape(rows, nx),
                                    counts=cnt.reshape(rows, nx), converged=conv.reshape(rows, nx))
    st["where"] = _masks(where, nx, rows)
    return st


# ---- frames with more than 256 partial sums -------------------------------------------------------------------------------------------
def tail_pixels(loc):
    """The image-order (row, column) of the pixels whose local index is above 65536 — the ones only the second trip of the final loop
    reaches — in local order."""
    flat = np.flatnonzero(loc.reshape(-1) > 65536)
    flat = flat[np.argsort(loc.reshape(-1)[flat])]
    return np.stack(np.unravel_index(flat, loc.shape), axis=1)


def big_state(nx, rows, loc, kind, seed=5, frame_id=0):
    """A frame of more than 65536 pixels with its extremes in tail_pixels(loc), so that a final loop that stops after one trip changes what
    it returns.  kind "uniform": done = 24, the largest V of the frame (a hundred times the sum of all others) and a tenth of the frame's
    luminance in two tail pixels.  "counts": done = 2^32 - 1; the one active pixel (the maximum count), the minimum count 2 and the
    largest V in tail pixels, every other count in [3, 2^31].  "nan": the uniform state with the frame's only NaN in a tail pixel."""
    rng = np.random.default_rng([seed, nx, rows])
    npix = nx * rows
    tail = tail_pixels(loc)
    assert len(tail) >= 4
    px = [tuple(p) for p in tail[[1, len(tail) // 3, len(tail) // 2, len(tail) - 1]]]
    y = rng.uniform(0.05, 1.0, (rows, nx))
    s = y * rng.uniform(0.02, 0.5, (rows, nx))
    total = rng.uniform(0.05, 4.0, (rows, nx, 3)).astype(F32)
    where = {"tail": np.zeros((rows, nx), bool)}
    where["tail"][tail[:, 0], tail[:, 1]] = True
    if kind == "counts":
        done = 2 ** 32 - 1
        cnt = rng.choice(rng.integers(3, 2 ** 31 + 1, 61), (rows, nx)).astype(np.uint32)  # (61 distinct counts)
        conv = np.ones((rows, nx), np.uint8)
        cnt[px[0]], conv[px[0]] = done, 0
        cnt[px[1]] = 2
    else:
        done, cnt, conv = 24, np.full((rows, nx), 24, np.uint32), None
    dn = cnt.astype(np.float64)
    s1, s2 = dn * y, dn * (y * y + s * s)
    ybar, v = adaptive_ref.pixel_figures(s1, s2, cnt)
    big_v = 100.0 * float(v.sum())
    n2 = float(cnt[px[2]])
    s1[px[2]], s2[px[2]] = n2 * 0.5, n2 * 0.25 + big_v * n2 * n2 * (n2 - 1.0) / n2
    s1[px[3]] = float(cnt[px[3]]) * 0.1 * float(ybar.sum())
    s2[px[3]] = s1[px[3]] * s1[px[3]] / float(cnt[px[3]]) * 1.0001
    if kind == "nan":
        s1[px[1]] = NAN64
    st = accum_state_ref.make_state(nx, rows, 0, done, frame_id, total, s1, s2, counts=cnt if conv is not None else None, converged=conv)
    st["where"], st["pixels"] = where, dict(active=px[0], min_count=px[1], largest_v=px[2], bright=px[3])
    return st


# ---- the order of the four waves ------------------------------------------------------------------------------------------------------
WAVE_TERMS = (1.0, 2.0 ** -53, 0.75 * 2.0 ** -52)  # ((1 + 2^-53) + 0.75 * 2^-52) = 1 + 2^-52, but ((1 + 0.75 * 2^-52) + 2^-53) = 1 + 2^-51
WAVE_SUM, WAVE_SUM_SWAPPED = 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -51


def wave_order_state(nx, rows, loc, frame_id=0):
    """A uniform state of two samples whose only non-zero figures sit in the first workgroup of the local pixel order: Ybar = WAVE_TERMS
    in the first pixel of waves 0, 2 and 3, V = WAVE_TERMS in their second pixel.  ((w0 + w1) + w2) + w3 is WAVE_SUM; with w2 and w3
    exchanged it is WAVE_SUM_SWAPPED.  Every other partial sum is 0, so the frame's sums are those of this workgroup."""
    s1, s2 = np.zeros((rows, nx)), np.zeros((rows, nx))
    flat = np.argsort(loc.reshape(-1))  # local index -> image-order index
    for wave, term in zip((0, 2, 3), WAVE_TERMS):
        at = np.unravel_index(flat[64 * wave], loc.shape)
        s1[at], s2[at] = 2.0 * term, 2.0 * term * term   # Ybar = term, S2 - S1 S1 / 2 = 0: V = 0
        at = np.unravel_index(flat[64 * wave + 1], loc.shape)
        s2[at] = 2.0 * term                              # S1 = 0: V = S2 / (2 - 1) / 2 = term
    total = np.full((rows, nx, 3), 0.5, F32)
    return accum_state_ref.make_state(nx, rows, 0, 2, frame_id, total, s1, s2)


# ---- a pixel that stopped on fewer than two samples -------------------------------------------------------------------------------------
def stopped_early_state(nx, rows, seed=13, frame_id=0):
    """An adaptive state of 8 issued samples with channel moments, every pixel noisy (a standard deviation of 8 times its mean, so that
    neighbours weight each other whatever their means), and two converged pixels in its interior that hold 0 and 1 samples — states no
    accumulation exports and rt_accum_state_check accepts.  Their pixel_noise figures are (0, 0) and (S1, 0): a finite guide."""
    rng = np.random.default_rng([seed, nx, rows])
    n = 8
    y = rng.uniform(0.2, 0.4, (rows, nx))
    s = 8.0 * y
    total = rng.uniform(0.5, 2.0, (rows, nx, 3)).astype(F32)
    cnt, conv = np.full((rows, nx), n, np.uint32), np.zeros((rows, nx), np.uint8)
    chm = np.zeros((rows, nx, 6))
    for ch in range(3):
        m = total[..., ch].astype(np.float64) / n
        chm[..., 2 * ch], chm[..., 2 * ch + 1] = n * m, n * (m * m + 64.0 * m * m)
    where = {}
    for count, at in ((0, (rows // 2, nx // 4)), (1, (rows // 2, 3 * nx // 4))):
        cnt[at], conv[at] = count, 1
        where["count %d" % count] = np.zeros((rows, nx), bool)
        where["count %d" % count][at] = True
    st = accum_state_ref.make_state(nx, rows, 0, n, frame_id, total, n * y, n * (y * y + s * s), counts=cnt, converged=conv, channel_moments=chm)
    st["where"] = where
    return st
