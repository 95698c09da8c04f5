// rt_channels.h — per-channel moments of an accumulation and the colour-guided filter (rtow_mi355x.h "Channel moments and the
// colour-guided filter"): new kernels only; no kernel of rt_kernels.h, rt_adaptive.h or rt_denoise.h changes.
//
//   k_resolve_moments_channels<ACTIVE> : k_resolve_moments<ACTIVE> plus S1_c += x_c, S2_c += x_c x_c per channel
//   k_channel_sem<COUNTS>              : (float)sqrt(V_c) per pixel and channel, in image order
//   k_denoise_inputs_channels<COUNTS>  : (c_ch, v_ch) per pixel and channel, in image order
//   k_denoise_channels<F>              : the filter; k_denoise<F> with three (c, v) planes in LDS and the channel-summed term in the map
//
// The channel moments are three planes of double2 (S1_c, S2_c), plane c at chm + c * npix, each in the local pixel order of the
// accumulation's sum: a lane reads and writes 16 B at stride 16 B per plane.  COUNTS: the pixel's own n_p (an adaptive accumulation).
#pragma once
#include "rt_denoise.h"

namespace rt {

// One sample of one pixel onto the eight f64 chains and the three f32 sums, in the order of k_resolve_moments.
struct ChannelSums {
    float r, g, b;
    double2 m, mr, mg, mb;
};
__device__ __forceinline__ void channel_sums_add(ChannelSums& a, float sx, float sy, float sz) {
    a.r += sx;
    a.g += sy;
    a.b += sz;
    const double y = sample_luminance(sx, sy, sz);
    a.m.x += y;
    a.m.y += y * y;
    const double dx = (double)sx, dy = (double)sy, dz = (double)sz;
    a.mr.x += dx, a.mr.y += dx * dx;
    a.mg.x += dy, a.mg.y += dy * dy;
    a.mb.x += dz, a.mb.y += dz * dz;
}

// The loads of four samples are issued before the first of their additions: behind each load of the rolled loop stands the dependent
// f64 chain of its sample, and with eight chains per pixel the kernel would wait for memory once per sample.  Every sum still takes
// its samples in sample order.  The remainder (s_count % 4 samples) goes one by one.
template <bool ACTIVE>
__global__ __launch_bounds__(256) void k_resolve_moments_channels(const float* __restrict__ rad, float* __restrict__ acc, double2* __restrict__ mom,
                                                                  double2* __restrict__ chm, const uint8_t* __restrict__ flag,
                                                                  uint32_t* __restrict__ cnt, uint32_t npix, uint32_t s_count) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npix) return;
    if (ACTIVE && flag[p] != 0u) return;
    ChannelSums a;
    a.r = acc[3 * (size_t)p], a.g = acc[3 * (size_t)p + 1], a.b = acc[3 * (size_t)p + 2];
    a.m = mom[p];
    a.mr = chm[p], a.mg = chm[(size_t)npix + p], a.mb = chm[2 * (size_t)npix + p];
    const size_t stride = (size_t)RT_RAD_FLOATS * npix;
    const float* src = rad + RT_RAD_FLOATS * (size_t)p;
    uint32_t s = 0;
    for (; s + 4u <= s_count; s += 4u, src += 4 * stride) {
        const float* s1 = src + stride;
        const float* s2 = s1 + stride;
        const float* s3 = s2 + stride;
        const float x0 = src[0], y0 = src[1], z0 = src[2];
        const float x1 = s1[0], y1 = s1[1], z1 = s1[2];
        const float x2 = s2[0], y2 = s2[1], z2 = s2[2];
        const float x3 = s3[0], y3 = s3[1], z3 = s3[2];
        channel_sums_add(a, x0, y0, z0);
        channel_sums_add(a, x1, y1, z1);
        channel_sums_add(a, x2, y2, z2);
        channel_sums_add(a, x3, y3, z3);
    }
    for (; s < s_count; ++s, src += stride) channel_sums_add(a, src[0], src[1], src[2]);
    acc[3 * (size_t)p] = a.r, acc[3 * (size_t)p + 1] = a.g, acc[3 * (size_t)p + 2] = a.b;
    mom[p] = a.m;
    chm[p] = a.mr, chm[(size_t)npix + p] = a.mg, chm[2 * (size_t)npix + p] = a.mb;
    if (ACTIVE) cnt[p] += s_count;
}

// V_c of "Channel moments": pixel_noise's variance of the mean on one channel's moments.
__device__ __forceinline__ double channel_variance(double2 m, uint32_t n) {
    double mean, v;
    pixel_noise(m, n, mean, v);
    return v;
}

// out_sem_rgb in output pixel order, as k_sem maps out_sem.
template <bool COUNTS>
__global__ __launch_bounds__(256) void k_channel_sem(const double2* __restrict__ chm, const uint32_t* __restrict__ cnt, float* __restrict__ out,
                                                     uint32_t nx, uint32_t rows, uint32_t n, uint32_t tiles_per_row, uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const uint32_t npix = nx * rows;
    if (p >= npix) return;
    const size_t ap = local_of_pixel(nx, tiles_per_row, tile_pixels, p % nx, p / nx);
    if (COUNTS) n = cnt[ap];
    for (uint32_t ch = 0; ch < 3u; ++ch) out[3 * (size_t)p + ch] = (float)sqrt(channel_variance(chm[(size_t)ch * npix + ap], n));
}

// The filter's inputs after n samples (COUNTS: n_p of the pixel), in image order: cv[3 p + ch] = (sum_ch / (float)n, (float)V_ch).
template <bool COUNTS>
__global__ __launch_bounds__(256) void k_denoise_inputs_channels(const float* __restrict__ sum, const double2* __restrict__ chm,
                                                                 const uint32_t* __restrict__ cnt, float2* __restrict__ cv, uint32_t nx, uint32_t rows,
                                                                 uint32_t n, uint32_t tiles_per_row, uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const uint32_t npix = nx * rows;
    if (p >= npix) return;
    const size_t ap = local_of_pixel(nx, tiles_per_row, tile_pixels, p % nx, p / nx);
    if (COUNTS) n = cnt[ap];
    const float fs = (float)n;
    for (uint32_t ch = 0; ch < 3u; ++ch)
        cv[3 * (size_t)p + ch] = make_float2(sum[3 * ap + ch] / fs, (float)channel_variance(chm[(size_t)ch * npix + ap], n));
}

// d_ch(a, b) of the header: a, b = (c_ch, v_ch) of two pixels — denoise_distance on a channel's mean and variance.
// k_denoise<F> (rt_denoise.h: the tile, the shared terms, the double-buffered map, one barrier per delta) with these differences:
//   - the tile is three planes of float2 (c_ch, v_ch), each at pitch RT_DN_PITCH, so the bank argument of RT_DN_PITCH holds per plane;
//   - a map entry is e = (d_r + d_g) + d_b: the three divisions are paid (16 + 2F)^2 times per delta, the patch sum of a pixel costs
//     what it costs in k_denoise;
//   - c_q of the numerator is the .x of the tile entry of q (q lies in the image: its entry is unclamped), c_p of the fall-back the .x
//     of p's own: no global load inside the delta loop.
// Grid and block as k_denoise<F>; dynamic LDS: denoise_channels_lds_bytes(R, F).
template <int F>
__global__ __launch_bounds__(256) void k_denoise_channels(const float2* __restrict__ cv, float* __restrict__ out, uint32_t nx, uint32_t rows, int R,
                                                          float k2) {
    extern __shared__ float2 dnc_tile[];
    constexpr int T = (int)RT_DN_TILE, TP = (int)RT_DN_PITCH, MP = (int)RT_DN_MAP_PITCH;
    constexpr int E = T + 2 * F; // side of the distance map
    const int H = R + F;
    const int side = T + 2 * H;
    const int plane = TP * side;
    float* const dmap = reinterpret_cast<float*>(dnc_tile + 3 * plane); // 2 buffers of MP * E floats
    const int x0 = (int)(blockIdx.x * RT_DN_TILE) - H, y0 = (int)(blockIdx.y * RT_DN_TILE) - H;
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    const int tid = ty * T + tx;
    for (int e = tid; e < side * side; e += 256) {
        const int ly = e / side, lx = e - ly * side;
        const int gx = min(max(x0 + lx, 0), (int)nx - 1), gy = min(max(y0 + ly, 0), (int)rows - 1);
        const float2* src = cv + 3 * ((size_t)gy * nx + gx);
        float2* dst = dnc_tile + ly * TP + lx;
        dst[0] = src[0], dst[plane] = src[1], dst[2 * plane] = src[2];
    }
    __syncthreads();
    const int px = (int)(blockIdx.x * RT_DN_TILE) + tx, py = (int)(blockIdx.y * RT_DN_TILE) + ty;
    const bool live = px < (int)nx && py < (int)rows;
    // the map entries this thread evaluates: e0 = tid and, for the E * E - 256 first threads, e1 = tid + 256 (E * E <= 484 < 512)
    const int m0y = tid / E, m0x = tid - m0y * E;
    const int e1 = tid + 256;
    const bool two = e1 < E * E;
    const int m1y = two ? e1 / E : 0, m1x = two ? e1 - m1y * E : 0;
    const float2* const a0p = dnc_tile + (m0y + R) * TP + m0x + R; // map entry (mx, my) is x = tile origin - F + (mx, my): tile entry + R
    const float2* const a1p = dnc_tile + (m1y + R) * TP + m1x + R;
    const float2 a0r = a0p[0], a0g = a0p[plane], a0b = a0p[2 * plane];
    const float2 a1r = a1p[0], a1g = a1p[plane], a1b = a1p[2 * plane];
    const float2* const me = dnc_tile + (ty + H) * TP + tx + H; // the tile entry of p
    constexpr float cnt3 = (float)(3 * (2 * F + 1) * (2 * F + 1));
    float den = 0.0f, nr = 0.0f, ng = 0.0f, nb = 0.0f;
    int buf = 0;
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = py + dy;
        for (int dx = -R; dx <= R; ++dx, buf ^= 1) {
            float* const map = dmap + buf * (MP * E);
            const int off = dy * TP + dx;
            map[m0y * MP + m0x] = (denoise_distance(a0r, a0p[off], k2) + denoise_distance(a0g, a0p[plane + off], k2)) +
                                  denoise_distance(a0b, a0p[2 * plane + off], k2);
            if (two)
                map[m1y * MP + m1x] = (denoise_distance(a1r, a1p[off], k2) + denoise_distance(a1g, a1p[plane + off], k2)) +
                                      denoise_distance(a1b, a1p[2 * plane + off], k2);
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
            const float D = S / cnt3;
            const float m = D < 0.0f ? 0.0f : D; // (a NaN stays one)
            float u = 1.0f - 0.25f * m;
            u = u > 0.0f ? u : 0.0f;             // (a NaN becomes 0)
            if (u != 0.0f) {
                const float w = (u * u) * (u * u);
                den = den + w;
                nr = nr + w * me[off].x, ng = ng + w * me[plane + off].x, nb = nb + w * me[2 * plane + off].x;
            }
        }
    }
    if (!live) return;
    const size_t p = (size_t)py * nx + px;
    float r = me[0].x, g = me[plane].x, b = me[2 * plane].x; // den == 0: p itself is not finite and stays what it is
    if (den != 0.0f) r = nr / den, g = ng / den, b = nb / den;
    out[3 * p] = r, out[3 * p + 1] = g, out[3 * p + 2] = b;
}
// dynamic LDS of k_denoise_channels<F>: the three (c, v) planes and the two distance maps; 39 168 B at R 5, F 1, 56 832 B at R 10, F 3
__host__ inline size_t denoise_channels_lds_bytes(uint32_t R, uint32_t F) {
    return 3u * (size_t)RT_DN_PITCH * (RT_DN_TILE + 2u * (R + F)) * sizeof(float2) + 2u * RT_DN_MAP_PITCH * (RT_DN_TILE + 2u * F) * sizeof(float);
}

} // namespace rt
