// rt_filter.h — the pixel reconstruction filters of an accumulation (rtow_mi355x.h "Pixel reconstruction filters"): new kernels only; no
// kernel of rt_kernels.h, rt_adaptive.h, rt_halves.h, rt_buckets.h or rt_accum_state_kernels.h changes, and none of these is in a variant
// table or a ledger family.
//
//   k_resolve_filter<ACTIVE, D> : the slice's samples onto the plane (sum w rgb, sum w) of every pixel, gathered from the pixel's own
//                                 radiance slots and those of its neighbours within the reach D
//   k_filter_read<COUNTS>       : sum.rgb / sum.w and sum.w in image order, the box mean where !(sum.w > 0)
// (rt_accum_export_filter and _import_filter move the plane as a PlaneTable row through k_planes_move, rt_accum_state_kernels.h.)
//
// k_resolve_filter.  A workgroup owns a 32 x 8 block of image pixels, lane t the pixel (t & 31, t >> 5) of it — whatever the local pixel
// order: every slot and every plane entry is found through local_of_pixel, so tiles, the row-major tail under them and frames without
// tiles take one path.  Per sample the workgroup stages its block plus a halo of D pixels into LDS, one staged slot per lane and trip:
// the radiance of the slot (one 12 B load) and the two jitters of its path, i.e. the two fmix32 rounds of path_key that depend on the sample
// and the draws of counters 0 and 1 (the round over the pixel is hoisted out of the sample loop) — once per slot, not once per
// (pixel, neighbour) pair.  Five planes of W x H floats (r, g, b, jx, jy): the 32 lanes of a row read 32 consecutive dwords of a plane, so
// the ds_read_b32 of a half wave touches every bank once.  The 256-entry table lies in LDS beside them; its two reads per neighbour go
// where the jitter sends them (conflicts there are data dependent).  Two buffers take turns, so one barrier per sample orders both the
// staging of sample s against its gather and the gather of s against the staging of s + 2.  A slot outside the frame, or of a converged
// pixel (ACTIVE), is staged with a jitter of 1e30: every lane skips it by the test that skips a sample outside the support.
// The additions a pixel sees are those of the header, in its order: samples ascending, dy ascending, dx ascending; -ffp-contract=off.
#pragma once
#include "rt_accum_state_kernels.h"
#include "rt_filter_plan.h"

namespace rt {

struct FilterArgs {
    const float* table;   // [RT_FILTER_TABLE]
    float4* plane;        // [npix], local pixel order
    const uint8_t* flag;  // ACTIVE: the converged flags, local pixel order
    uint32_t nx, rows, npix, tiles_per_row, tile_pixels;
    uint32_t seed_lo, seed_hi;
    uint32_t i0, s_count; // the absolute index of the slice's first sample, and how many it holds
    float radius, scale;  // R and pixel_filter_scale(R)
};

constexpr uint32_t RT_FILTER_BLOCK_X = 32u, RT_FILTER_BLOCK_Y = 8u;
constexpr float RT_FILTER_NO_SAMPLE = 1e30f; // the jitter of a slot that holds no sample: beyond every radius

template <bool ACTIVE, int D>
__global__ __launch_bounds__(256) void k_resolve_filter(const float* __restrict__ rad, FilterArgs a) {
    constexpr int W = (int)RT_FILTER_BLOCK_X + 2 * D, H = (int)RT_FILTER_BLOCK_Y + 2 * D, N = W * H, NS = (N + 255) / 256;
    __shared__ float s_tab[RT_FILTER_TABLE];
    __shared__ float s_v[2][5][N];
    const uint32_t t = threadIdx.x, tx = t & 31u, ty = t >> 5;
    const int x0 = (int)(blockIdx.x * RT_FILTER_BLOCK_X), y0 = (int)(blockIdx.y * RT_FILTER_BLOCK_Y);
    s_tab[t] = a.table[t]; // (the first barrier of the sample loop orders it)

    // the slots this lane stages for every sample: where their radiance lies and the sample-independent round of their key
    uint32_t slot_local[NS], slot_key[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int slot = (int)t + 256 * k;
        slot_local[k] = 0xFFFFFFFFu, slot_key[k] = 0u;
        if (slot >= N) continue;
        const int qi = x0 + slot % W - D, qj = y0 + slot / W - D;
        if (qi < 0 || qj < 0 || qi >= (int)a.nx || qj >= (int)a.rows) continue;
        const uint32_t lq = local_of_pixel(a.nx, a.tiles_per_row, a.tile_pixels, (uint32_t)qi, (uint32_t)qj);
        if (ACTIVE && a.flag[lq] != 0u) continue; // nothing wrote its radiance slots
        slot_local[k] = lq;
        slot_key[k] = fmix32(((uint32_t)qj * a.nx + (uint32_t)qi) ^ a.seed_lo); // `a` of path_key
    }

    const uint32_t pi = (uint32_t)x0 + tx, pj = (uint32_t)y0 + ty;
    const bool mine = pi < a.nx && pj < a.rows;
    const uint32_t lp = mine ? local_of_pixel(a.nx, a.tiles_per_row, a.tile_pixels, pi, pj) : 0u;
    float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (mine) sum = a.plane[lp];
    const float R = a.radius, scale = a.scale;

    for (uint32_t s = 0; s < a.s_count; ++s) {
        float(*v)[N] = s_v[s & 1u];
        const uint32_t samp = a.i0 + s;
        const float* src = rad + (size_t)RT_RAD_FLOATS * ((size_t)s * a.npix);
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int slot = (int)t + 256 * k;
            if (slot >= N) continue;
            float r = 0.0f, g = 0.0f, b = 0.0f, jx = RT_FILTER_NO_SAMPLE, jy = RT_FILTER_NO_SAMPLE;
            if (slot_local[k] != 0xFFFFFFFFu) {
                const float* q = src + (size_t)RT_RAD_FLOATS * slot_local[k];
                r = q[0], g = q[1], b = q[2];
                const uint32_t ka = slot_key[k]; // path_key, then the draws of counters 0 and 1 as gen_primary makes them
                const uint32_t k0 = fmix32(ka + samp * 0x9E3779B9u + a.seed_hi), k1 = fmix32((ka ^ 0xA511E9B3u) + samp * 0xC2B2AE3Du);
                Rng rng(k0, k1, 0u);
                jx = rng.next(), jy = rng.next();
            }
            v[0][slot] = r, v[1][slot] = g, v[2][slot] = b, v[3][slot] = jx, v[4][slot] = jy;
        }
        __syncthreads();
        if (!mine) continue;
#pragma unroll
        for (int dy = -D; dy <= D; ++dy) {
#pragma unroll
            for (int dx = -D; dx <= D; ++dx) {
                const int sl = ((int)ty + D + dy) * W + (int)tx + D + dx;
                const float ox = ((float)dx + v[3][sl]) - 0.5f, oy = ((float)dy + v[4][sl]) - 0.5f;
                const float ax = fabsf(ox), ay = fabsf(oy);
                if (ax > R || ay > R) continue;
                // min((uint32_t)(ax * scale), 255): the clamp in f32 first gives the same index and converts no value out of range
                const uint32_t kx = (uint32_t)fminf(ax * scale, (float)(RT_FILTER_TABLE - 1u)), ky = (uint32_t)fminf(ay * scale, (float)(RT_FILTER_TABLE - 1u));
                const float w = s_tab[kx] * s_tab[ky];
                sum.x += w * v[0][sl];
                sum.y += w * v[1][sl];
                sum.z += w * v[2][sl];
                sum.w += w;
            }
        }
    }
    if (mine) a.plane[lp] = sum;
}

// rt_accum_read_filtered: c = sum.rgb / sum.w and W = sum.w in image order; where !(W > 0) the box mean acc / (float)max(n, 1) of
// k_finalize.  COUNTS: n is the pixel's own n_p (an adaptive accumulation); otherwise `n` as passed, and `cnt` is not read.  Either output
// may be NULL.
template <bool COUNTS>
__global__ __launch_bounds__(256) void k_filter_read(const float4* __restrict__ plane, const float* __restrict__ acc, const uint32_t* __restrict__ cnt,
                                                     float* __restrict__ out_rgb, float* __restrict__ out_w, uint32_t nx, uint32_t rows, uint32_t n,
                                                     uint32_t tiles_per_row, uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx * rows) return;
    const size_t ap = local_of_pixel(nx, tiles_per_row, tile_pixels, p % nx, p / nx);
    const float4 s = plane[ap];
    StateRgb c{s.x / s.w, s.y / s.w, s.z / s.w};
    if (!(s.w > 0.0f)) {
        if (COUNTS) n = cnt[ap];
        const float fs = (float)(n ? n : 1u);
        const StateRgb b = reinterpret_cast<const StateRgb*>(acc)[ap];
        c = StateRgb{b.r / fs, b.g / fs, b.b / fs};
    }
    if (out_rgb) reinterpret_cast<StateRgb*>(out_rgb)[p] = c;
    if (out_w) out_w[p] = s.w;
}

} // namespace rt
