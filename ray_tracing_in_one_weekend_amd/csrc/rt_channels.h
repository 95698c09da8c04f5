// rt_channels.h — per-channel moments of an accumulation and the colour-guided filter (rtow_mi355x.h "Channel moments and the
// colour-guided filter"): new kernels only; no kernel of rt_kernels.h, rt_adaptive.h or rt_denoise.h changes.
//
//   k_resolve_moments_channels<ACTIVE> : k_resolve_moments<ACTIVE> plus S1_c += x_c, S2_c += x_c x_c per channel
//   k_channel_sem<COUNTS>              : (float)sqrt(V_c) per pixel and channel, in image order
//   k_denoise_inputs_channels<COUNTS>  : (c_ch, v_ch) per pixel and channel, in image order
//   k_denoise_channels<F>              : nlm_filter<F, GuideChannels> (rt_denoise.h): three (c, v) planes in LDS, the channel-summed term in the map
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

// GuideChannels: d_ch(a, b) of the header is denoise_distance on a channel's mean and variance, and the filter is nlm_filter
// (rt_denoise.h: the tile, the shared terms, the double-buffered map, one barrier per delta) with the three differences its constants name:
//   - the tile is three planes of float2 (c_ch, v_ch);
//   - a map entry is e = (d_r + d_g) + d_b: the three divisions are paid (16 + 2F)^2 times per delta, the patch sum of a pixel costs
//     what it costs in k_denoise;
//   - c_q of the numerator is the .x of the tile entry of q, c_p of the fall-back the .x of p's own: no global load inside the delta loop.
struct GuideChannels {
    static constexpr int PLANES = 3;
    static constexpr bool COLOUR_IN_TILE = true;
};
// Grid and block as k_denoise<F>; dynamic LDS: nlm_lds_bytes(3, R, F).
template <int F>
__global__ __launch_bounds__(256) void k_denoise_channels(const float2* __restrict__ cv, float* __restrict__ out, uint32_t nx, uint32_t rows, int R,
                                                          float k2) {
    nlm_filter<F, GuideChannels>(nullptr, cv, out, nx, rows, R, k2);
}

} // namespace rt
