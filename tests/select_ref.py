"""Reference for "Selected strength" of rtow_mi355x.h in numpy, on top of halves_ref (the inputs, the combine, l), denoise_ref.denoise (the
unchanged filter) and noise_tree_ref (the tree of the frame figures): the K candidates, E_j, the usable mask, B_j by row sums first, the
choice, W_j, the blend, est and the RtSelectInfo — f32 step by step, every operation one IEEE operation in the header's order.  Also the
designed inputs the tests feed it."""
import numpy as np

import denoise_ref
import halves_ref
import noise_tree_ref

F32 = np.float32
NAN32 = halves_ref.NAN32
FOUR_STRENGTHS = (0.45, 0.7, 1.0, 1.4)  # the candidates the designed inputs are built for (with S 2, T 1); the library's defaults are three


def _clamped(n, halo):
    return np.clip(np.arange(-halo, n + halo), 0, n - 1)


def window_sums(E, usable, S):
    """(B [rows, nx] f32, U [rows, nx] int): B(p) = sum_oy (sum_ox E(clamp(p + o))), row sums first, each from +0, the terms of pixels that
    are not usable skipped; U the number of usable terms."""
    rows, nx = E.shape
    ys, xs = _clamped(rows, S), _clamped(nx, S)
    Ex, Ux = E[:, xs], usable[:, xs]
    row, cnt = np.zeros((rows, nx), F32), np.zeros((rows, nx), np.int64)
    with np.errstate(all="ignore"):
        for ox in range(2 * S + 1):
            use = Ux[:, ox:ox + nx]
            row = np.where(use, row + Ex[:, ox:ox + nx], row)
            cnt = cnt + use
        Ry, Cy = row[ys], cnt[ys]
        B, U = np.zeros((rows, nx), F32), np.zeros((rows, nx), np.int64)
        for oy in range(2 * S + 1):
            B = B + Ry[oy:oy + rows]
            U = U + Cy[oy:oy + rows]
    assert B.dtype == F32
    return B, U


def choose(B):
    """s [rows, nx] and best = B_s: from K - 1 downwards, a smaller B takes over (ties stay with the larger j; a NaN never takes over)."""
    K = len(B)
    s, best = np.full(B[0].shape, K - 1, np.int64), B[K - 1]
    for j in range(K - 2, -1, -1):
        take = B[j] < best
        s, best = np.where(take, j, s), np.where(take, B[j], best)
    return s, best


def blend(outs, s, T):
    """(out, W [K, rows, nx]): W_j = the count of j in the clamped (2T + 1)^2 window of s; out = (the W-weighted sum of out_j in increasing j,
    W_j != 0 only, starting with its first term) / (float)((2T + 1)^2)."""
    K, (rows, nx) = len(outs), s.shape
    sp = s[_clamped(rows, T)][:, _clamped(nx, T)]
    W = np.zeros((K, rows, nx), np.int64)
    for oy in range(2 * T + 1):
        for ox in range(2 * T + 1):
            win = sp[oy:oy + rows, ox:ox + nx]
            for j in range(K):
                W[j] += win == j
    acc, have = np.zeros((rows, nx, 3), F32), np.zeros((rows, nx), bool)
    with np.errstate(all="ignore"):
        for j in range(K):
            term = W[j].astype(F32)[..., None] * outs[j]
            on = W[j] != 0
            acc = np.where((on & have)[..., None], acc + term, np.where(on[..., None], term, acc))
            have |= on
        out = acc / F32((2 * T + 1) * (2 * T + 1))
    assert out.dtype == F32 and have.all()
    return out, W


def info(E, usable, s):
    """The RtSelectInfo as a dict: f64 sums over the pixels in image order on the tree of noise_tree_ref (a pixel that is not usable adds 0.0)."""
    K = len(E)
    n = int(usable.sum())
    flat = lambda a: np.where(usable, a.astype(np.float64), 0.0).reshape(-1)
    Es = np.choose(s, E)
    with np.errstate(all="ignore"):
        est = [float(np.float64(noise_tree_ref.tree_sum(flat(E[j]))) / np.float64(n)) for j in range(K)]
        sel = float(np.float64(noise_tree_ref.tree_sum(flat(Es))) / np.float64(n))
    best = K - 1
    for j in range(K - 2, -1, -1):
        if est[j] < est[best]:
            best = j
    return dict(est_mse=est + [0.0] * (4 - K), est_mse_selected=sel, chosen=[int((s == j).sum()) for j in range(K)] + [0] * (4 - K), usable=n, best=best)


def candidates(ins, nh, strengths, radius, patch):
    """Steps 1 and 2 for every strength: (outs [K] = out_j, E [K] = E_j, f [K][2] = f_{j,h})."""
    outs, E, fs = [], [], []
    for k in strengths:
        f = [denoise_ref.denoise(ins[h][0], ins[1 - h][1], ins[1 - h][2], radius, patch, k)[0] for h in range(2)]
        o, _ = halves_ref.combine(f[0], f[1], nh[0], nh[1])
        with np.errstate(all="ignore"):
            e = []
            for h in range(2):
                r = halves_ref.lum32(f[h]) - np.asarray(ins[1 - h][1], F32)
                e.append(r * r - np.asarray(ins[1 - h][2], F32))
            Ej = F32(0.5) * (e[0] + e[1])
        assert Ej.dtype == F32
        outs.append(o), E.append(Ej), fs.append(f)
    return outs, E, fs


def finish(cands, S, T, K=None):
    """Steps 3 to 5 and the figures over the first K candidates of `cands` (a candidate does not depend on the others).  Returns a dict:
    out, rgb8, index, est, info, outs [K], E [K], usable, B [K], U, W [K, rows, nx], f [K][2]."""
    outs, E, fs = (x[:K] for x in cands)
    usable = np.all([np.isfinite(e) for e in E], axis=0)
    BU = [window_sums(e, usable, S) for e in E]
    B, U = [b for b, _ in BU], BU[0][1]
    s, best = choose(B)
    with np.errstate(all="ignore"):
        est = np.where(U == 0, NAN32, best / U.astype(F32)).astype(F32)
    out, W = blend(outs, s, T)
    return dict(out=out, index=s.astype(np.uint8), est=est, info=info(E, usable, s), outs=outs, E=E, usable=usable, B=B, U=U, W=W, f=fs,
                rgb8=denoise_ref.finalize_rgb8(out))


def select_inputs(ins, nh, strengths, radius, patch, S, T):
    """ins = [(c_0, y_0, v_0), (c_1, y_1, v_1)] in image order, nh = [n_0, n_1] (ints or [rows, nx] arrays)."""
    return finish(candidates(ins, nh, strengths, radius, patch), S, T)


def state_inputs(halves, first_sample, n):
    """(ins, nh) of a designed state: halves [(sum, S1, S2)] x 2 in image order; n: done, or the per-pixel counts."""
    nh = [halves_ref.n_h(first_sample, n, h) for h in range(2)]
    return [halves_ref.inputs(*halves[h], nh[h]) for h in range(2)], nh


def select(halves, first_sample, n, strengths=FOUR_STRENGTHS, radius=5, patch=1, S=2, T=1):
    """halves: [(sum, S1, S2)] x 2 in image order; n: done, or the per-pixel counts — as halves_ref.cross_filter takes them."""
    ins, nh = state_inputs(halves, first_sample, n)
    return dict(select_inputs(ins, nh, strengths, radius, patch, S, T), inputs=ins, nh=nh)


def info_matches(got, want):
    """The RtSelectInfo `got` (ctypes) against the dict `want`: f64 figures by their bits (a NaN is a NaN), the integers exactly."""
    same = lambda a, b: (a != a and b != b) or np.float64(a).tobytes() == np.float64(b).tobytes()
    return (all(same(a, b) for a, b in zip(got.est_mse, want["est_mse"])) and same(got.est_mse_selected, want["est_mse_selected"]) and
            list(got.chosen) == want["chosen"] and got.usable == want["usable"] and got.best == want["best"] and list(got.reserved) == [0, 0])


# ---- designed inputs: (halves, first_sample, done, counts or None) ----------------------------------------------------------------------------
def synthetic_halves():
    """64 x 48, two halves of 8 heavy-tailed samples (seeds 7 and 8): every one of the four candidates wins somewhere and the blend mixes."""
    return halves_ref.plain_halves(64, 48), 0, 16, None


def kernel_halves():
    """37 x 21 with a v = 0 block, a NaN and a +inf pixel in half 0: exact ties, pixels that are not usable, windows with 0 < U < (2S + 1)^2."""
    return halves_ref.kernel_halves(37, 21), 0, 16, None


def adaptive_state(first=4):
    """37 x 21 with pixels of 0 .. 3 samples spread over the frame (halves_ref.adaptive_counts): those with an n_h < 2 are not usable."""
    cnt, conv = halves_ref.adaptive_counts(37, 21)
    return halves_ref.plain_halves(37, 21, nh=4), first, 8, cnt, conv


def blind_state():
    """19 x 12 with a 7 x 7 block of one-sample pixels: with S <= 2 the windows in its middle hold no usable pixel (U = 0, est NaN)."""
    cnt, conv = np.full((12, 19), 8, np.uint32), np.zeros((12, 19), np.uint8)
    cnt[3:10, 5:12], conv[3:10, 5:12] = 1, 1
    return halves_ref.plain_halves(19, 12, nh=4), 0, 8, cnt, conv
