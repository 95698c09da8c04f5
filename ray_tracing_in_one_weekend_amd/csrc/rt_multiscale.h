// rt_multiscale.h — the kernels around the filter in "Multi-scale denoising" (rtow_mi355x.h): a 2x pyramid whose every level is filtered by
// the unchanged nlm_filter (rt_denoise.h, rt_channels.h) and whose coarser levels replace the low frequencies of the finer ones.
//
//   k_ms_down<PLANES> : level s -> s + 1 of the filter's inputs; PLANES 1: c and (y, v) apart, PLANES 3: (c, v) x 3 as dn_cv holds them
//   k_ms_residual     : e = o_{s+1} - D(F_s) per coarse pixel and channel, a non-finite e replaced by +0
//   k_ms_up_add       : o_s = F_s + U(e) per fine pixel and channel, U the 2x bilinear interpolation at pixel centres
//
// All three stream a few bytes per pixel in image order: one thread per pixel of the level they write, p = blockIdx.x * 256 + threadIdx.x,
// so consecutive lanes take consecutive pixels of a row and a wave reads and writes whole runs of a row.  A colour triple goes as three
// dword accesses per lane at c[3 p + ch], the way k_denoise_inputs writes them: the three together cover the wave's 768 B without a gap.
// Every operation is one IEEE f32 operation in the header's order (-ffp-contract=off); tests/denoise_multiscale_ref.py restates them in
// numpy and the kernels are held to it bit for bit.  Every multiplier of D is a power of two, so its scale is exact.
#pragma once
#include "rt_kernels.h"

namespace rt {

// What a coarse pixel (X, Y) of a level with nx x rows pixels below it reads: its four taps' pixel indices, which of them lie in the
// image, and the two scales.  k = kx ky in {1, 2, 4} taps inside: a mean takes 1 / k, a variance of a mean of k means 1 / (k k).
struct MsTaps {
    size_t p00, p10, p01, p11;
    bool in_x, in_y;
    float mean, var;
};
__device__ __forceinline__ MsTaps ms_taps(uint32_t X, uint32_t Y, uint32_t nx, uint32_t rows) {
    MsTaps t;
    t.in_x = 2u * X + 1u < nx, t.in_y = 2u * Y + 1u < rows;
    t.p00 = (size_t)(2u * Y) * nx + 2u * X;
    t.p10 = t.p00 + 1u, t.p01 = t.p00 + nx, t.p11 = t.p01 + 1u;
    t.mean = t.in_x ? (t.in_y ? 0.25f : 0.5f) : (t.in_y ? 0.5f : 1.0f);
    t.var = t.mean * t.mean; // 1, 0.25 or 0.0625: exact
    return t;
}
// (t00 + t10) + (t01 + t11) of the plane `a` with the stride `stride` floats per pixel; a tap outside the image is +0.0f
__device__ __forceinline__ float ms_sum(const float* __restrict__ a, const MsTaps& t, uint32_t stride, uint32_t at) {
    const float t00 = a[stride * t.p00 + at];
    const float t10 = t.in_x ? a[stride * t.p10 + at] : 0.0f;
    const float t01 = t.in_y ? a[stride * t.p01 + at] : 0.0f;
    const float t11 = t.in_x && t.in_y ? a[stride * t.p11 + at] : 0.0f;
    return (t00 + t10) + (t01 + t11);
}

// The inputs of level s + 1 (nx1 x rows1 = the halves, rounded up, of nx x rows) from those of level s.  PLANES 1: c [3 per pixel] and
// g = (y, v) [1 float2 per pixel]; PLANES 3: g = (c_ch, v_ch) [3 float2 per pixel], c and c1 are not used.
template <int PLANES>
__global__ __launch_bounds__(256) void k_ms_down(const float* __restrict__ c, const float2* __restrict__ g, float* __restrict__ c1, float2* __restrict__ g1,
                                                 uint32_t nx, uint32_t rows, uint32_t nx1, uint32_t rows1) {
    static_assert(PLANES == 1 || PLANES == 3, "one plane of (y, v) beside the colours, or three of (c, v)");
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx1 * rows1) return;
    const MsTaps t = ms_taps(p % nx1, p / nx1, nx, rows);
    const float* const gf = reinterpret_cast<const float*>(g);
    if constexpr (PLANES == 1) {
        for (uint32_t ch = 0; ch < 3u; ++ch) c1[3 * (size_t)p + ch] = ms_sum(c, t, 3u, ch) * t.mean;
        g1[p] = make_float2(ms_sum(gf, t, 2u, 0u) * t.mean, ms_sum(gf, t, 2u, 1u) * t.var);
    } else {
        for (uint32_t ch = 0; ch < 3u; ++ch)
            g1[3 * (size_t)p + ch] = make_float2(ms_sum(gf, t, 6u, 2u * ch) * t.mean, ms_sum(gf, t, 6u, 2u * ch + 1u) * t.var);
    }
}

// e [3 per pixel of level s + 1] = o1 - D(f), D the mean form over the filtered level s (nx x rows); what is not finite becomes +0.0f
__global__ __launch_bounds__(256) void k_ms_residual(const float* __restrict__ o1, const float* __restrict__ f, float* __restrict__ e, uint32_t nx,
                                                     uint32_t rows, uint32_t nx1, uint32_t rows1) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx1 * rows1) return;
    const MsTaps t = ms_taps(p % nx1, p / nx1, nx, rows);
    for (uint32_t ch = 0; ch < 3u; ++ch) {
        const float d = o1[3 * (size_t)p + ch] - ms_sum(f, t, 3u, ch) * t.mean;
        e[3 * (size_t)p + ch] = (__float_as_uint(d) & 0x7F800000u) == 0x7F800000u ? 0.0f : d;
    }
}

// o [3 per pixel of level s, nx x rows] = f + U(e), e of level s + 1 (nx1 x rows1).  The pixel (x, y) lies a quarter of a coarse pixel
// from the centre of (X, Y) = (x >> 1, y >> 1), towards X + 1 where x is odd and towards X - 1 where it is even: the weights 3/4 and 1/4
// per axis, their products 9/16, 3/16, 3/16, 1/16.  The neighbour is clamped at the border per axis.
__global__ __launch_bounds__(256) void k_ms_up_add(const float* __restrict__ f, const float* __restrict__ e, float* __restrict__ o, uint32_t nx, uint32_t rows,
                                                   uint32_t nx1, uint32_t rows1) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx * rows) return;
    const uint32_t x = p % nx, y = p / nx;
    const int X = (int)(x >> 1), Y = (int)(y >> 1);
    const int X2 = min(max(X + ((x & 1u) ? 1 : -1), 0), (int)nx1 - 1), Y2 = min(max(Y + ((y & 1u) ? 1 : -1), 0), (int)rows1 - 1);
    const float* const e00 = e + 3 * ((size_t)Y * nx1 + X);
    const float* const e10 = e + 3 * ((size_t)Y * nx1 + X2);
    const float* const e01 = e + 3 * ((size_t)Y2 * nx1 + X);
    const float* const e11 = e + 3 * ((size_t)Y2 * nx1 + X2);
    for (uint32_t ch = 0; ch < 3u; ++ch)
        o[3 * (size_t)p + ch] = f[3 * (size_t)p + ch] + ((0.5625f * e00[ch] + 0.1875f * e10[ch]) + (0.1875f * e01[ch] + 0.0625f * e11[ch]));
}

} // namespace rt
