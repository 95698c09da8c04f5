// rt_denoise.h — the variance-guided non-local-means filter of rt_accum_denoise (rtow_mi355x.h "Denoising"): image space, new kernels
// only, fed by what an accumulation already owns (the running f32 sum and the two f64 luminance moments per pixel).
//
//   k_denoise_inputs<COUNTS> : c = sum / (float)n, y = (float)Ybar, v = (float)V per pixel, in image order (COUNTS: n = the pixel's n_p)
//   nlm_filter<F, G> : the filter's body; one thread per pixel, the guide tile of a workgroup and its halo in LDS, the distance terms
//                      that the patches of neighbouring pixels share evaluated once per workgroup; G: the guide policy
//   k_denoise<F>     : nlm_filter<F, GuideLuminance>: one plane of (y, v), colours read from global memory
//
// Every operation of the filter is one IEEE f32 operation in the header's order (-ffp-contract=off, the compiler's correctly rounded
// `/`): tests/denoise_ref.py restates it in numpy and the kernel is held to it bit for bit.
#pragma once
#include "rt_kernels.h"

namespace rt {

constexpr uint32_t RT_DN_TILE = 16u; // a workgroup filters 16 x 16 pixels: 256 threads, four waves of four rows
// Pitch of the LDS tile in float2 entries.  A tile row is at most 16 + 2 (10 + 3) = 42 entries wide.  ds_read_b64 resolves bank conflicts
// per 32-lane half, bank = (byte address / 4) % 64; a half holds two tile rows of 16 lanes, 32 banks each, which fall on the two halves of
// the 64 banks exactly when the pitch is 16 mod 32 entries: 48 for every radius and patch, 48 * 42 * 8 B = 15.75 KiB at the most.
constexpr uint32_t RT_DN_PITCH = 48u;

// The filter's inputs of one accumulation after n samples, in image order (p = row * nx + column, row 0 at the bottom).
// COUNTS: with the pixel's own n_p (`n` is not used; otherwise `cnt` is not read).  There a pixel with n_p < 2 has no variance (only an
// imported state holds one beside done >= 2: rt_accum_state_check accepts a converged pixel with any counts[p] <= done): its c is what
// rt_accum_read returns, sum / (float)max(n_p, 1), and its guide is NaN, so that it stays what it is and spreads to no other pixel.
template <bool COUNTS>
__global__ __launch_bounds__(256) void k_denoise_inputs(const float* __restrict__ sum, const double2* __restrict__ mom, const uint32_t* __restrict__ cnt,
                                                        float* __restrict__ c, float2* __restrict__ yv, uint32_t nx, uint32_t rows, uint32_t n,
                                                        uint32_t tiles_per_row, uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx * rows) return;
    const size_t ap = local_of_pixel(nx, tiles_per_row, tile_pixels, p % nx, p / nx);
    if (COUNTS) n = cnt[ap];
    const float fs = (float)(COUNTS && n == 0u ? 1u : n);
    c[3 * (size_t)p] = sum[3 * ap] / fs, c[3 * (size_t)p + 1] = sum[3 * ap + 1] / fs, c[3 * (size_t)p + 2] = sum[3 * ap + 2] / fs;
    double ybar, v;
    pixel_noise(mom[ap], n, ybar, v);
    const float none = __uint_as_float(0x7FC00000u);
    yv[p] = COUNTS && n < 2u ? make_float2(none, none) : make_float2((float)ybar, (float)v);
}

// d(a, b) of the header: a, b = (y, v) of two pixels
__device__ __forceinline__ float denoise_distance(float2 a, float2 b, float k2) {
    const float dy = a.x - b.x;
    const float vmin = b.y < a.y ? b.y : a.y; // min(v_a, v_b); either being NaN makes the quotient NaN whichever is picked
    return (dy * dy - (a.y + vmin)) / (1e-10f + k2 * (a.y + b.y));
}

// Pitch of the distance map in floats.  ds_read_b32 banks are (byte address / 4) % 32 within a 32-lane half, two rows of 16 lanes: 16 mod 32
// puts them on the two halves of the banks; a map row is at most 16 + 2 * 3 = 22 wide.
constexpr uint32_t RT_DN_MAP_PITCH = 48u;

// What guides the filter, a compile-time policy of constants that answers the three things in which the two filters differ and nothing
// else.  PLANES: how many float2 planes (mean, variance) the tile holds, 1 or 3; plane ch of a tile entry lies ch * plane entries behind
// plane 0.  With it what a map entry is: d of the one plane, or (d_0 + d_1) + d_2, and the divisor PLANES times the patch's pixels.
// COLOUR_IN_TILE: channel ch of a pixel's colour is the .x of plane ch of its tile entry; otherwise c[3 * pixel + ch] in global memory.
// (Constants, not functions: the compiler simplifies a policy's function on its own before it inlines it, without the body around it,
// and the kernels then come out as other, if equivalent, code than the text written out in one piece gives.)
// GuideLuminance: one plane of (y, v); colours from global memory.  (GuideChannels: rt_channels.h.)
struct GuideLuminance {
    static constexpr int PLANES = 1;
    static constexpr bool COLOUR_IN_TILE = false;
};

// The non-local-means body of k_denoise<F> and k_denoise_channels<F>.  g: G::PLANES entries (mean, variance) per pixel in image order.
// F: the patch radius (0 .. RT_DENOISE_MAX_PATCH), a template parameter so that the patch loops unroll.  R: 1 .. RT_DENOISE_MAX_RADIUS.
// Grid: ceil(nx / 16) x ceil(rows / 16) workgroups of 16 x 16 threads; dynamic LDS: nlm_lds_bytes(G::PLANES, R, F).
//
// The tile.  LDS entry (lx, ly) of a plane holds (mean, v) of the pixel clamp(x0 - H + lx), clamp(y0 - H + ly), H = R + F, each axis
// clamped on its own: the clamped patch coordinates of the header ARE the entries at p + o and q + o, since q itself lies in the image
// (so its entry is unclamped).  Every plane has the pitch RT_DN_PITCH, so its bank argument holds per plane.
//
// Shared terms.  The term of offset o in the patch distance of (p, q = p + delta) is e(x, delta) = d(clamp(x), clamp(x + delta)) with
// x = p + o, summed over the planes: a function of x and delta alone, and the same term for the (2F + 1)^2 pixels p = x - o.  So per
// delta the workgroup evaluates e ONCE for every x of its tile grown by F — (16 + 2F)^2 terms, each with its division per plane, instead
// of 256 (2F + 1)^2 — into a map in LDS, and a pixel sums its (2F + 1)^2 entries in the header's order (rows first): the same operands in
// the same order, the same bits.  The map is double-buffered, so one barrier per delta is enough: a thread that runs ahead writes the
// other buffer, and reaches the buffer being read only behind the next barrier, which every reader has then passed.  Every thread of the
// workgroup walks all deltas (the barriers), whether its pixel or its q lies in the image or not; only the accumulation is guarded.
template <int F, class G>
__device__ __forceinline__ void nlm_filter(const float* c, const float2* g, float* out, uint32_t nx, uint32_t rows, int R, float k2) {
    extern __shared__ float2 dn_tile[];
    constexpr int T = (int)RT_DN_TILE, TP = (int)RT_DN_PITCH, MP = (int)RT_DN_MAP_PITCH, P = G::PLANES;
    static_assert(P == 1 || P == 3, "the map entry is written out for one plane and for three");
    constexpr int E = T + 2 * F; // side of the distance map
    const int H = R + F;
    const int side = T + 2 * H;
    const int plane = TP * side;
    float* const dmap = reinterpret_cast<float*>(dn_tile + P * plane); // 2 buffers of MP * E floats
    const int x0 = (int)(blockIdx.x * RT_DN_TILE) - H, y0 = (int)(blockIdx.y * RT_DN_TILE) - H;
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    const int tid = ty * T + tx;
    for (int e = tid; e < side * side; e += 256) {
        const int ly = e / side, lx = e - ly * side;
        const int gx = min(max(x0 + lx, 0), (int)nx - 1), gy = min(max(y0 + ly, 0), (int)rows - 1);
        const float2* src = g + P * ((size_t)gy * nx + gx);
        float2* dst = dn_tile + ly * TP + lx;
        for (int ch = 0; ch < P; ++ch) dst[ch * plane] = src[ch];
    }
    __syncthreads();
    const int px = (int)(blockIdx.x * RT_DN_TILE) + tx, py = (int)(blockIdx.y * RT_DN_TILE) + ty;
    const bool live = px < (int)nx && py < (int)rows;
    // the map entries this thread evaluates: e0 = tid and, for the E * E - 256 first threads, e1 = tid + 256 (E * E <= 484 < 512)
    const int m0y = tid / E, m0x = tid - m0y * E;
    const int e1 = tid + 256;
    const bool two = e1 < E * E;
    const int m1y = two ? e1 / E : 0, m1x = two ? e1 - m1y * E : 0;
    const float2* const a0p = dn_tile + (m0y + R) * TP + m0x + R; // map entry (mx, my) is x = tile origin - F + (mx, my): tile entry + R
    const float2* const a1p = dn_tile + (m1y + R) * TP + m1x + R;
    const float2 a0 = a0p[0], a0g = a0p[P == 3 ? plane : 0], a0b = a0p[P == 3 ? 2 * plane : 0]; // (one plane: a0g, a0b are not used)
    const float2 a1 = a1p[0], a1g = a1p[P == 3 ? plane : 0], a1b = a1p[P == 3 ? 2 * plane : 0];
    const float2* const me = dn_tile + (ty + H) * TP + tx + H; // the tile entry of p
    constexpr float cnt = (float)(P * (2 * F + 1) * (2 * F + 1));
    float den = 0.0f, nr = 0.0f, ng = 0.0f, nb = 0.0f;
    int buf = 0;
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = py + dy;
        for (int dx = -R; dx <= R; ++dx, buf ^= 1) {
            float* const map = dmap + buf * (MP * E);
            const int off = dy * TP + dx;
            if constexpr (P == 1) {
                map[m0y * MP + m0x] = denoise_distance(a0, a0p[off], k2);
                if (two) map[m1y * MP + m1x] = denoise_distance(a1, a1p[off], k2);
            } else {
                map[m0y * MP + m0x] = (denoise_distance(a0, a0p[off], k2) + denoise_distance(a0g, a0p[plane + off], k2)) +
                                      denoise_distance(a0b, a0p[2 * plane + off], k2);
                if (two)
                    map[m1y * MP + m1x] = (denoise_distance(a1, a1p[off], k2) + denoise_distance(a1g, a1p[plane + off], k2)) +
                                          denoise_distance(a1b, a1p[2 * plane + off], k2);
            }
            __syncthreads();
            const int qx = px + dx;
            if (!live || qy < 0 || qy >= (int)rows || qx < 0 || qx >= (int)nx) continue;
            const float* const mine = map + (ty + F) * MP + tx + F; // the map entry of x = p
            float S = 0.0f;
            for (int oy = -F; oy <= F; ++oy) {
                float row = 0.0f;
                for (int ox = -F; ox <= F; ++ox) row = row + mine[oy * MP + ox];
                S = S + row;
            }
            const float D = S / cnt;
            const float m = D < 0.0f ? 0.0f : D; // (a NaN stays one)
            float u = 1.0f - 0.25f * m;
            u = u > 0.0f ? u : 0.0f;             // (a NaN becomes 0)
            if (u != 0.0f) {
                const float w = (u * u) * (u * u);
                den = den + w;
                if constexpr (G::COLOUR_IN_TILE) {
                    nr = nr + w * me[off].x, ng = ng + w * me[plane + off].x, nb = nb + w * me[2 * plane + off].x;
                } else {
                    const float* cq = c + 3 * ((size_t)qy * nx + qx);
                    nr = nr + w * cq[0], ng = ng + w * cq[1], nb = nb + w * cq[2];
                }
            }
        }
    }
    if (!live) return;
    const size_t p = (size_t)py * nx + px;
    float r, gr, b; // den == 0: p itself is not finite and stays what it is
    if constexpr (G::COLOUR_IN_TILE) r = me[0].x, gr = me[plane].x, b = me[2 * plane].x;
    else r = c[3 * p], gr = c[3 * p + 1], b = c[3 * p + 2];
    if (den != 0.0f) r = nr / den, gr = ng / den, b = nb / den;
    out[3 * p] = r, out[3 * p + 1] = gr, out[3 * p + 2] = b;
}
// dynamic LDS of the filter: `planes` tiles and the two distance maps.  R 5, F 1: 17 664 B with one plane, 39 168 B with three; R 10, F 3, the
// maximum: 24 576 B and 56 832 B
__host__ inline size_t nlm_lds_bytes(uint32_t planes, uint32_t R, uint32_t F) {
    return planes * (size_t)RT_DN_PITCH * (RT_DN_TILE + 2u * (R + F)) * sizeof(float2) + 2u * RT_DN_MAP_PITCH * (RT_DN_TILE + 2u * F) * sizeof(float);
}

template <int F>
__global__ __launch_bounds__(256) void k_denoise(const float* __restrict__ c, const float2* __restrict__ yv, float* __restrict__ out,
                                                 uint32_t nx, uint32_t rows, int R, float k2) {
    nlm_filter<F, GuideLuminance>(c, yv, out, nx, rows, R, k2);
}

} // namespace rt
