// rt_select.h — the strength of the cross filter chosen per pixel from the half buffers (rtow_mi355x.h "Selected strength"): new kernels
// only, around the unchanged k_denoise<F> of rt_denoise.h and the inputs of rt_halves.h; none of them is in a variant table or a ledger family.
// Per candidate j the host launches k_denoise<F> twice (each half by the other's guide, as rt_accum_denoise_halves does) — the plain chain —
// or k_denoise_multi<F, K> once per half for all candidates — the fused chain, the same bits — and then
//
//   k_select_error<COUNTS> : f_{j,0}, f_{j,1}, the guides and the counts -> out_j (the combine of k_halves_combine) and E_j
//   k_select_choose        : a tile of the K error planes and the usable mask with an S halo in LDS, separable sums, rows first -> s, est
//   k_select_partials      : per 256 pixels in image order, the f64 sums of E_j and E_s over the usable pixels and the integer counts
//   k_select_blend         : a tile of indices with a T halo in LDS -> out
//   k_select_final         : one workgroup over the partials -> RtSelectInfo
//
// Everything is in image order (p = row * nx + column, row 0 at the bottom).  Every operation is one IEEE f32 operation in the header's
// order (-ffp-contract=off): tests/select_ref.py restates it in numpy and the kernels are held to it bit for bit.
#pragma once
#include "rt_denoise.h"
#include "rt_halves.h"
#include "rt_select_plan.h"

namespace rt {

// The K planes of a run, by candidate.
struct SelectPlanes {
    float* out_j[RT_SELECT_MAX]; // [npix * 3]
    float* e_j[RT_SELECT_MAX];   // [npix]
};

// out_j = combine(f_0, f_1) as k_halves_combine; E_j = 0.5f ((l(f_0) - y_1)^2 - v_1 + (l(f_1) - y_0)^2 - v_0), each half against the OTHER
// half's guide, the independent picture of the truth.  A guide of a half with n_h < 2 is NaN (k_denoise_inputs_halves): E_j is NaN there.
template <bool COUNTS>
__global__ __launch_bounds__(256) void k_select_error(const float* __restrict__ f0, const float* __restrict__ f1, const float2* __restrict__ yv0,
                                                      const float2* __restrict__ yv1, const uint32_t* __restrict__ cnt, float* __restrict__ out,
                                                      float* __restrict__ err, uint32_t nx, uint32_t rows, uint32_t first, uint32_t n,
                                                      uint32_t tiles_per_row, uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx * rows) return;
    const HalfPixel hx = half_pixel<COUNTS>(cnt, p, nx, first, n, tiles_per_row, tile_pixels);
    const StateRgb x0 = reinterpret_cast<const StateRgb*>(f0)[p], x1 = reinterpret_cast<const StateRgb*>(f1)[p];
    const float a0 = (float)hx.n[0], a1 = (float)hx.n[1];
    StateRgb o{halves_mix(x0.r, x1.r, a0, a1), halves_mix(x0.g, x1.g, a0, a1), halves_mix(x0.b, x1.b, a0, a1)};
    if (hx.n[1] == 0u) o = x0;
    else if (hx.n[0] == 0u) o = x1;
    reinterpret_cast<StateRgb*>(out)[p] = o;
    const float2 g0 = yv0[p], g1 = yv1[p];
    const float r0 = halves_luminance(x0) - g1.x, r1 = halves_luminance(x1) - g0.x;
    const float e0 = r0 * r0 - g1.y, e1 = r1 * r1 - g0.y;
    err[p] = 0.5f * (e0 + e1);
}

// ---- the fused chain: one filter launch per half for all K strengths ----------------------------------------------------------------------------
// k_denoise_multi<F, K> is nlm_filter<F, GuideLuminance> (rt_denoise.h) with K strengths at once: the tile, the barriers, the colour loads
// and, of d(a, b) = (dy dy - (v_a + min(v_a, v_b))) / (eps + k2 (v_a + v_b)), the numerator and v_a + v_b are shared between the candidates;
// K divisions, K distance maps and K sets of accumulators remain.  Per candidate the operands and their order are those of k_denoise<F>, so
// it gives the plain chain's bits (tests/test_select.py).  The K maps lie behind each other in LDS, each double-buffered, each with
// rt_denoise.h's pitch RT_DN_MAP_PITCH, so its bank argument holds per map: a 32-lane half reads two map rows of 16 floats, 16 mod 32 apart.
struct SelectMulti {
    float* out[RT_SELECT_MAX]; // f_{j,h} of this half, [npix * 3] each
    float k2[RT_SELECT_MAX];   // k_j * k_j
};
__host__ inline size_t select_multi_lds_bytes(uint32_t K, uint32_t R, uint32_t F) {
    return (size_t)RT_DN_PITCH * (RT_DN_TILE + 2u * (R + F)) * sizeof(float2) + (size_t)K * 2u * RT_DN_MAP_PITCH * (RT_DN_TILE + 2u * F) * sizeof(float);
}
template <int F, int K>
__global__ __launch_bounds__(256) void k_denoise_multi(const float* __restrict__ c, const float2* __restrict__ g, SelectMulti sm, uint32_t nx, uint32_t rows, int R) {
    extern __shared__ float2 dn_tile[];
    constexpr int T = (int)RT_DN_TILE, TP = (int)RT_DN_PITCH, MP = (int)RT_DN_MAP_PITCH;
    constexpr int E = T + 2 * F; // side of a distance map
    constexpr int MAP = MP * E;  // floats of one buffer of one map
    const int H = R + F;
    const int side = T + 2 * H;
    float* const dmap = reinterpret_cast<float*>(dn_tile + TP * side); // K maps of 2 buffers of MAP floats: map j, buffer b at (2 j + b) MAP
    const int x0 = (int)(blockIdx.x * RT_DN_TILE) - H, y0 = (int)(blockIdx.y * RT_DN_TILE) - H;
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    const int tid = ty * T + tx;
    for (int e = tid; e < side * side; e += 256) {
        const int ly = e / side, lx = e - ly * side;
        const int gx = min(max(x0 + lx, 0), (int)nx - 1), gy = min(max(y0 + ly, 0), (int)rows - 1);
        dn_tile[ly * TP + lx] = g[(size_t)gy * nx + gx];
    }
    __syncthreads();
    const int px = (int)(blockIdx.x * RT_DN_TILE) + tx, py = (int)(blockIdx.y * RT_DN_TILE) + ty;
    const bool live = px < (int)nx && py < (int)rows;
    const int m0y = tid / E, m0x = tid - m0y * E;
    const int e1 = tid + 256;
    const bool two = e1 < E * E;
    const int m1y = two ? e1 / E : 0, m1x = two ? e1 - m1y * E : 0;
    const float2* const a0p = dn_tile + (m0y + R) * TP + m0x + R;
    const float2* const a1p = dn_tile + (m1y + R) * TP + m1x + R;
    const float2 a0 = a0p[0], a1 = a1p[0];
    constexpr float cnt = (float)((2 * F + 1) * (2 * F + 1));
    float den[K], nr[K], ng[K], nb[K];
#pragma unroll
    for (int j = 0; j < K; ++j) den[j] = nr[j] = ng[j] = nb[j] = 0.0f;
    int buf = 0;
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = py + dy;
        for (int dx = -R; dx <= R; ++dx, buf ^= 1) {
            float* const map = dmap + buf * MAP;
            const int off = dy * TP + dx;
            {
                const float2 b = a0p[off];
                const float d = a0.x - b.x;
                const float vmin = b.y < a0.y ? b.y : a0.y;
                const float num = d * d - (a0.y + vmin), vs = a0.y + b.y;
#pragma unroll
                for (int j = 0; j < K; ++j) map[2 * j * MAP + m0y * MP + m0x] = num / (1e-10f + sm.k2[j] * vs);
            }
            if (two) {
                const float2 b = a1p[off];
                const float d = a1.x - b.x;
                const float vmin = b.y < a1.y ? b.y : a1.y;
                const float num = d * d - (a1.y + vmin), vs = a1.y + b.y;
#pragma unroll
                for (int j = 0; j < K; ++j) map[2 * j * MAP + m1y * MP + m1x] = num / (1e-10f + sm.k2[j] * vs);
            }
            __syncthreads();
            const int qx = px + dx;
            if (!live || qy < 0 || qy >= (int)rows || qx < 0 || qx >= (int)nx) continue;
            const float* const cq = c + 3 * ((size_t)qy * nx + qx);
            const float cr = cq[0], cg = cq[1], cb = cq[2];
            const float* const mine = map + (ty + F) * MP + tx + F;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                float S = 0.0f;
                for (int oy = -F; oy <= F; ++oy) {
                    float row = 0.0f;
                    for (int ox = -F; ox <= F; ++ox) row = row + mine[2 * j * MAP + oy * MP + ox];
                    S = S + row;
                }
                const float D = S / cnt;
                const float m = D < 0.0f ? 0.0f : D;
                float u = 1.0f - 0.25f * m;
                u = u > 0.0f ? u : 0.0f;
                if (u != 0.0f) {
                    const float w = (u * u) * (u * u);
                    den[j] = den[j] + w;
                    nr[j] = nr[j] + w * cr, ng[j] = ng[j] + w * cg, nb[j] = nb[j] + w * cb;
                }
            }
        }
    }
    if (!live) return;
    const size_t p = (size_t)py * nx + px;
    const float pr = c[3 * p], pg = c[3 * p + 1], pb = c[3 * p + 2];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        float r = pr, gr = pg, b = pb; // den == 0: p itself is not finite and stays what it is
        if (den[j] != 0.0f) r = nr[j] / den[j], gr = ng[j] / den[j], b = nb[j] / den[j];
        float* const o = sm.out[j];
        o[3 * p] = r, o[3 * p + 1] = gr, o[3 * p + 2] = b;
    }
}

__device__ __forceinline__ bool select_finite(float x) { return x - x == 0.0f; }

// Pitch of a row of the LDS tiles in floats: RT_SEL_SIDE_MAX = 24 entries at the most.  A 32-lane half reads two tile rows of 16 consecutive
// floats; with a pitch of 16 mod 32 — 48, as rt_denoise.h's map — they fall on the two halves of the 32 banks ds_read_b32 resolves conflicts over.
constexpr uint32_t RT_SEL_PITCH = 48u;

// Grid: ceil(nx / 16) x ceil(rows / 16) workgroups of 16 x 16 threads.  Static LDS: K_MAX error planes and the mask of the tile with its
// halo (5 * 24 * 48 * 4 B = 23 040 B) and the row sums of K_MAX planes and of the mask (5 * 24 * 16 * 4 B = 7 680 B).
// Tile entry (lx, ly) holds the pixel (clamp(x0 - S + lx), clamp(y0 - S + ly)), each axis clamped on its own, so the clamped window of the
// header IS the (2S + 1)^2 entries around a pixel's own.  Row sums first: rs_j(x, ly) = sum over ox in order of the usable E_j(x + ox, ly),
// evaluated once per workgroup for the 16 columns and 16 + 2S rows — every pixel of a column shares them — then B_j(p) = sum over oy in
// order of rs_j(px, py + oy): the same operands in the same order as the header's double loop.
__global__ __launch_bounds__(256) void k_select_choose(SelectPlanes pl, uint32_t K, int S, uint8_t* __restrict__ index, float* __restrict__ est,
                                                       uint32_t nx, uint32_t rows) {
    constexpr int T = (int)RT_SEL_TILE, SM = (int)RT_SEL_SIDE_MAX, TP = (int)RT_SEL_PITCH, KM = (int)RT_SELECT_MAX;
    __shared__ float tile[KM][SM * TP];
    __shared__ uint32_t mask[SM * TP];
    __shared__ float rs[KM][SM * T];
    __shared__ uint32_t ru[SM * T];
    const int side = T + 2 * S;
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y, tid = ty * T + tx;
    for (int e = tid; e < side * side; e += 256) {
        const int ly = e / side, lx = e - ly * side;
        const size_t q = (size_t)select_clamp(blockIdx.y, (uint32_t)ly, (uint32_t)S, rows) * nx + select_clamp(blockIdx.x, (uint32_t)lx, (uint32_t)S, nx);
        bool ok = true;
        for (uint32_t j = 0; j < K; ++j) {
            const float v = pl.e_j[j][q];
            tile[j][ly * TP + lx] = v;
            ok = ok && select_finite(v);
        }
        mask[ly * TP + lx] = ok ? 1u : 0u;
    }
    __syncthreads();
    for (int e = tid; e < side * T; e += 256) { // the row sums of column cx of the 16, tile row ly
        const int ly = e / T, cx = e - ly * T;
        const int at = ly * TP + cx + S; // the tile entry of (cx, ly): its window runs from at - S to at + S
        uint32_t u = 0u;
        for (int ox = -S; ox <= S; ++ox) u += mask[at + ox];
        ru[e] = u;
        for (uint32_t j = 0; j < K; ++j) {
            float row = 0.0f;
            for (int ox = -S; ox <= S; ++ox)
                if (mask[at + ox]) row = row + tile[j][at + ox];
            rs[j][e] = row;
        }
    }
    __syncthreads();
    const uint32_t px = blockIdx.x * RT_SEL_TILE + tx, py = blockIdx.y * RT_SEL_TILE + ty;
    if (px >= nx || py >= rows) return;
    uint32_t U = 0u;
    for (int oy = -S; oy <= S; ++oy) U += ru[(ty + S + oy) * T + tx];
    uint32_t s = K - 1u;
    float best = 0.0f;
    for (uint32_t jj = 0; jj < K; ++jj) {
        const uint32_t j = K - 1u - jj;
        float B = 0.0f;
        for (int oy = -S; oy <= S; ++oy) B = B + rs[j][(ty + S + oy) * T + tx];
        if (jj == 0u) best = B;
        else if (B < best) s = j, best = B;
    }
    const size_t p = (size_t)py * nx + px;
    index[p] = (uint8_t)s;
    est[p] = U ? best / (float)U : __uint_as_float(0x7FC00000u);
}

// partials[workgroup]: the sums of its 256 pixels in image order by block_sum_256 (a pixel that is not usable and a tail slot add 0.0), and
// the integer counts (exact in any order: LDS integer atomics).
__global__ __launch_bounds__(256) void k_select_partials(SelectPlanes pl, uint32_t K, const uint8_t* __restrict__ index, SelectPartial* __restrict__ partials,
                                                         uint32_t npix) {
    __shared__ double2 part[3][4];
    __shared__ uint32_t cnt[RT_SELECT_MAX + 1u];
    if (threadIdx.x <= RT_SELECT_MAX) cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    double e[RT_SELECT_MAX + 2u] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; // E_0 .. E_3, E_s, (unused)
    if (p < npix) {
        const uint32_t s = index[p];
        float v[RT_SELECT_MAX] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool ok = true;
        for (uint32_t j = 0; j < RT_SELECT_MAX; ++j)
            if (j < K) v[j] = pl.e_j[j][p], ok = ok && select_finite(v[j]);
        atomicAdd(&cnt[s], 1u);
        if (ok) {
            atomicAdd(&cnt[RT_SELECT_MAX], 1u);
            for (uint32_t j = 0; j < RT_SELECT_MAX; ++j) e[j] = (double)v[j];
            e[RT_SELECT_MAX] = (double)(s == 0u ? v[0] : s == 1u ? v[1] : s == 2u ? v[2] : v[3]);
        }
    }
    const double2 s01 = block_sum_256(e[0], e[1], part[0]);
    const double2 s23 = block_sum_256(e[2], e[3], part[1]);
    const double2 s4 = block_sum_256(e[4], e[5], part[2]); // (its barrier also orders the counts before they are read)
    if (threadIdx.x != 0) return;
    SelectPartial out;
    out.e[0] = s01.x, out.e[1] = s01.y, out.e[2] = s23.x, out.e[3] = s23.y, out.e[4] = s4.x;
    for (uint32_t j = 0; j <= RT_SELECT_MAX; ++j) out.n[j] = cnt[j];
    out.pad = 0u;
    partials[blockIdx.x] = out;
}

// Grid and block as k_select_choose.  W_j = how many indices of the (2T + 1)^2 window around p, clamped per axis, are j; out = the W-weighted
// mean of the candidates in increasing j, candidates with W_j == 0 left out, the sum starting with its first term.
__global__ __launch_bounds__(256) void k_select_blend(SelectPlanes pl, uint32_t K, int Tr, const uint8_t* __restrict__ index, float* __restrict__ out,
                                                      uint32_t nx, uint32_t rows) {
    constexpr int T = (int)RT_SEL_TILE, SM = (int)RT_SEL_SIDE_MAX, TP = (int)RT_SEL_PITCH;
    __shared__ uint32_t tile[SM * TP];
    const int side = T + 2 * Tr;
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y, tid = ty * T + tx;
    for (int e = tid; e < side * side; e += 256) {
        const int ly = e / side, lx = e - ly * side;
        const size_t q = (size_t)select_clamp(blockIdx.y, (uint32_t)ly, (uint32_t)Tr, rows) * nx + select_clamp(blockIdx.x, (uint32_t)lx, (uint32_t)Tr, nx);
        tile[ly * TP + lx] = index[q];
    }
    __syncthreads();
    const uint32_t px = blockIdx.x * RT_SEL_TILE + tx, py = blockIdx.y * RT_SEL_TILE + ty;
    if (px >= nx || py >= rows) return;
    uint32_t W[RT_SELECT_MAX] = {0u, 0u, 0u, 0u};
    for (int oy = -Tr; oy <= Tr; ++oy)
        for (int ox = -Tr; ox <= Tr; ++ox) {
            const uint32_t s = tile[(ty + Tr + oy) * TP + tx + Tr + ox];
            W[0] += s == 0u, W[1] += s == 1u, W[2] += s == 2u, W[3] += s == 3u;
        }
    const size_t p = (size_t)py * nx + px;
    const float cnt = (float)select_window((uint32_t)Tr);
    float r = 0.0f, g = 0.0f, b = 0.0f;
    bool any = false;
    for (uint32_t j = 0; j < RT_SELECT_MAX; ++j) {
        if (j >= K || W[j] == 0u) continue;
        const StateRgb x = reinterpret_cast<const StateRgb*>(pl.out_j[j])[p];
        const float w = (float)W[j];
        const float tr = w * x.r, tg = w * x.g, tb = w * x.b;
        r = any ? r + tr : tr, g = any ? g + tg : tg, b = any ? b + tb : tb;
        any = true;
    }
    reinterpret_cast<StateRgb*>(out)[p] = StateRgb{r / cnt, g / cnt, b / cnt};
}

// One workgroup: thread t adds the partials t, t + 256, .. in index order, then block_sum_256 — the tree of k_noise_final — and thread 0
// writes the RtSelectInfo.
__global__ __launch_bounds__(256) void k_select_final(const SelectPartial* __restrict__ partials, uint32_t n_partials, uint32_t K, RtSelectInfo* __restrict__ info) {
    __shared__ double2 part[3][4];
    __shared__ uint32_t cnt[RT_SELECT_MAX + 1u];
    if (threadIdx.x <= RT_SELECT_MAX) cnt[threadIdx.x] = 0u;
    __syncthreads();
    double e[RT_SELECT_MAX + 2u] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t n[RT_SELECT_MAX + 1u] = {0u, 0u, 0u, 0u, 0u};
    for (uint32_t k = threadIdx.x; k < n_partials; k += 256u) {
        const SelectPartial sp = partials[k];
        for (uint32_t j = 0; j <= RT_SELECT_MAX; ++j) e[j] += sp.e[j], n[j] += sp.n[j];
    }
    for (uint32_t j = 0; j <= RT_SELECT_MAX; ++j)
        if (n[j]) atomicAdd(&cnt[j], n[j]);
    const double2 s01 = block_sum_256(e[0], e[1], part[0]);
    const double2 s23 = block_sum_256(e[2], e[3], part[1]);
    const double2 s4 = block_sum_256(e[4], e[5], part[2]);
    if (threadIdx.x != 0) return;
    const double sum[RT_SELECT_MAX] = {s01.x, s01.y, s23.x, s23.y};
    const double usable = (double)cnt[RT_SELECT_MAX];
    RtSelectInfo o{};
    for (uint32_t j = 0; j < RT_SELECT_MAX; ++j) {
        o.est_mse[j] = j < K ? sum[j] / usable : 0.0;
        o.chosen[j] = cnt[j];
    }
    o.est_mse_selected = s4.x / usable;
    o.usable = cnt[RT_SELECT_MAX];
    uint32_t best = K - 1u;
    for (uint32_t jj = 1; jj < K; ++jj) {
        const uint32_t j = K - 1u - jj;
        if (o.est_mse[j] < o.est_mse[best]) best = j;
    }
    o.best = best;
    *info = o;
}

} // namespace rt
