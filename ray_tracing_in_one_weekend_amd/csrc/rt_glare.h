// rt_glare.h — the kernels of "Glare" (rtow_mi355x.h): an energy-conserving bloom of the f32 image in front of the display stage.  A 2x
// pyramid of the bright pass is summed back up with one weight per level; the taps and scales of D are those of rt_multiscale.h
// (ms_taps, ms_sum), U is the interpolation of k_ms_up_add with its sum order.
//
//   k_glare_bright_down : c -> d_1: sanitise, bright pass and the first D in one pass; d_0 is never stored
//   k_glare_down        : d_l -> d_{l+1}
//   k_glare_down3       : c -> d_1, d_2 and d_3 in ONE launch (the fused down chain): a workgroup owns a tile of 64 x 16 fine pixels whose
//                         origin is a multiple of 8 on both axes, so every pixel of d_1 (32 x 8), d_2 (16 x 4) and d_3 (8 x 2) it writes
//                         depends on its own tile alone — no halo; d_1 and d_2 pass to the next level through LDS.  Each level takes its
//                         taps' validity and its 1 / k from the size of the level below it, as the plain kernels do: the same operations
//                         in the same order, the same bits.
//   k_glare_up          : u_l = w_l d_l + U(u_{l+1}) (the coarsest level: u_l = w_l d_l)
//   k_glare_combine     : out = (s - a b) + a U(u_1), s and b recomputed from c (12 B read again instead of 24 B stored and read)
//
// All stream a few bytes per pixel in image order, one thread per pixel they write (k_glare_down3: per pixel of d_1), a colour triple as
// three dword accesses per lane, the way the multi-scale kernels do.  Every f32 operation is one IEEE operation in the header's order
// (-ffp-contract=off); tests/glare_ref.py restates them in numpy and the kernels are held to it bit for bit.  GPU-free parts:
// rt_glare_plan.h.
#pragma once
#include "rt_display.h"
#include "rt_glare_plan.h"
#include "rt_multiscale.h"

namespace rt {

constexpr uint32_t RT_GLARE_TILE_X = 64u, RT_GLARE_TILE_Y = 16u; // fine pixels per workgroup of k_glare_down3
constexpr float RT_GLARE_CEILING = 18446744073709551616.0f;      // 0x1p64f

// Steps 1 and 2 of pixel p: s, the sanitised colour, and b, its bright pass.  Returns whether every channel of c is finite.
__device__ __forceinline__ bool glare_bright(const float* __restrict__ c, size_t p, float threshold, float s[3], float b[3], float raw[3]) {
    bool fin = true;
    for (int ch = 0; ch < 3; ++ch) {
        const float v = c[3 * p + ch];
        raw[ch] = v;
        const bool f = display_finite(v);
        fin = fin && f;
        s[ch] = (f && v > 0.0f) ? (v < RT_GLARE_CEILING ? v : RT_GLARE_CEILING) : 0.0f;
    }
    if (threshold == 0.0f) {
        for (int ch = 0; ch < 3; ++ch) b[ch] = s[ch];
    } else {
        const float Y = display_luminance(s[0], s[1], s[2]);
        const float k = Y > threshold ? (Y - threshold) / Y : 0.0f;
        for (int ch = 0; ch < 3; ++ch) b[ch] = s[ch] * k;
    }
    return fin;
}

// D of the bright pass at the coarse pixel whose taps are t: (t00 + t10) + (t01 + t11) per channel, a tap outside the image +0, times 1 / k
__device__ __forceinline__ void glare_bright_mean(const float* __restrict__ c, const MsTaps& t, float threshold, float out[3]) {
    float s[3], raw[3], b00[3], b10[3] = {0.0f, 0.0f, 0.0f}, b01[3] = {0.0f, 0.0f, 0.0f}, b11[3] = {0.0f, 0.0f, 0.0f};
    glare_bright(c, t.p00, threshold, s, b00, raw);
    if (t.in_x) glare_bright(c, t.p10, threshold, s, b10, raw);
    if (t.in_y) glare_bright(c, t.p01, threshold, s, b01, raw);
    if (t.in_x && t.in_y) glare_bright(c, t.p11, threshold, s, b11, raw);
    for (int ch = 0; ch < 3; ++ch) out[ch] = ((b00[ch] + b10[ch]) + (b01[ch] + b11[ch])) * t.mean;
}

// d1 [3 per pixel, nx1 x rows1] = D(b), b the bright pass of c [3 per pixel, nx x rows]
__global__ __launch_bounds__(256) void k_glare_bright_down(const float* __restrict__ c, float* __restrict__ d1, uint32_t nx, uint32_t rows, uint32_t nx1,
                                                           uint32_t rows1, float threshold) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx1 * rows1) return;
    float v[3];
    glare_bright_mean(c, ms_taps(p % nx1, p / nx1, nx, rows), threshold, v);
    for (uint32_t ch = 0; ch < 3u; ++ch) d1[3 * (size_t)p + ch] = v[ch];
}

// d1 [nx1 x rows1] = D(d) of d [nx x rows]
__global__ __launch_bounds__(256) void k_glare_down(const float* __restrict__ d, float* __restrict__ d1, uint32_t nx, uint32_t rows, uint32_t nx1, uint32_t rows1) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx1 * rows1) return;
    const MsTaps t = ms_taps(p % nx1, p / nx1, nx, rows);
    for (uint32_t ch = 0; ch < 3u; ++ch) d1[3 * (size_t)p + ch] = ms_sum(d, t, 3u, ch) * t.mean;
}

// The taps of the coarse pixel (X, Y) of a level over a tile of the level below it that lies in LDS, `width` pixels wide, the coarse pixel
// at (lx, ly) of its own tile: validity and scale from the level's size (nx x rows below it), the indices into the tile.
__device__ __forceinline__ MsTaps glare_tile_taps(uint32_t X, uint32_t Y, uint32_t nx, uint32_t rows, uint32_t lx, uint32_t ly, uint32_t width) {
    MsTaps t = ms_taps(X, Y, nx, rows);
    t.p00 = (size_t)(2u * ly) * width + 2u * lx;
    t.p10 = t.p00 + 1u, t.p01 = t.p00 + width, t.p11 = t.p01 + 1u;
    return t;
}

// The fused down chain: grid = tiles_x * tiles_y workgroups, tiles of RT_GLARE_TILE_X x RT_GLARE_TILE_Y pixels of c in row order of the tiles.
// (nx1, rows1) .. (nx3, rows3): the sizes of levels 1 .. 3.  A pixel of a level outside its image is neither computed nor stored; its
// slot in LDS holds +0 and no tap inside the image reads it.
__global__ __launch_bounds__(256) void k_glare_down3(const float* __restrict__ c, float* __restrict__ d1, float* __restrict__ d2, float* __restrict__ d3,
                                                     uint32_t nx, uint32_t rows, uint32_t nx1, uint32_t rows1, uint32_t nx2, uint32_t rows2, uint32_t nx3,
                                                     uint32_t rows3, uint32_t tiles_x, float threshold) {
    constexpr uint32_t W1 = RT_GLARE_TILE_X / 2u, H1 = RT_GLARE_TILE_Y / 2u, W2 = W1 / 2u, H2 = H1 / 2u, W3 = W2 / 2u, H3 = H2 / 2u;
    static_assert(W1 * H1 == 256u && RT_GLARE_TILE_X % 8u == 0u && RT_GLARE_TILE_Y % 8u == 0u, "one thread per pixel of d_1; tiles of whole 8 x 8 blocks");
    __shared__ float s1[W1 * H1 * 3u];
    __shared__ float s2[W2 * H2 * 3u];
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    {
        const uint32_t lx = threadIdx.x % W1, ly = threadIdx.x / W1, X = tx * W1 + lx, Y = ty * H1 + ly;
        float v[3] = {0.0f, 0.0f, 0.0f};
        if (X < nx1 && Y < rows1) {
            glare_bright_mean(c, ms_taps(X, Y, nx, rows), threshold, v);
            const size_t p = (size_t)Y * nx1 + X;
            for (uint32_t ch = 0; ch < 3u; ++ch) d1[3 * p + ch] = v[ch];
        }
        for (uint32_t ch = 0; ch < 3u; ++ch) s1[3u * threadIdx.x + ch] = v[ch];
    }
    __syncthreads();
    if (threadIdx.x < W2 * H2) {
        const uint32_t lx = threadIdx.x % W2, ly = threadIdx.x / W2, X = tx * W2 + lx, Y = ty * H2 + ly;
        float v[3] = {0.0f, 0.0f, 0.0f};
        if (X < nx2 && Y < rows2) {
            const MsTaps t = glare_tile_taps(X, Y, nx1, rows1, lx, ly, W1);
            const size_t p = (size_t)Y * nx2 + X;
            for (uint32_t ch = 0; ch < 3u; ++ch) d2[3 * p + ch] = v[ch] = ms_sum(s1, t, 3u, ch) * t.mean;
        }
        for (uint32_t ch = 0; ch < 3u; ++ch) s2[3u * threadIdx.x + ch] = v[ch];
    }
    __syncthreads();
    if (threadIdx.x < W3 * H3) {
        const uint32_t lx = threadIdx.x % W3, ly = threadIdx.x / W3, X = tx * W3 + lx, Y = ty * H3 + ly;
        if (X < nx3 && Y < rows3) {
            const MsTaps t = glare_tile_taps(X, Y, nx2, rows2, lx, ly, W2);
            const size_t p = (size_t)Y * nx3 + X;
            for (uint32_t ch = 0; ch < 3u; ++ch) d3[3 * p + ch] = ms_sum(s2, t, 3u, ch) * t.mean;
        }
    }
}

// U(e) at the pixel (x, y) of a level, e [3 per pixel] of the next coarser level (nx1 x rows1): the four taps and the sum order of
// k_ms_up_add — 9/16 to the coarse pixel that holds (x, y), 3/16 to its neighbour per axis on the side (x, y) lies, clamped, 1/16 diagonal.
struct GlareUp {
    const float *e00, *e10, *e01, *e11;
};
__device__ __forceinline__ GlareUp glare_up_taps(const float* __restrict__ e, uint32_t x, uint32_t y, uint32_t nx1, uint32_t rows1) {
    const int X = (int)(x >> 1), Y = (int)(y >> 1);
    const int X2 = min(max(X + ((x & 1u) ? 1 : -1), 0), (int)nx1 - 1), Y2 = min(max(Y + ((y & 1u) ? 1 : -1), 0), (int)rows1 - 1);
    return GlareUp{e + 3 * ((size_t)Y * nx1 + X), e + 3 * ((size_t)Y * nx1 + X2), e + 3 * ((size_t)Y2 * nx1 + X), e + 3 * ((size_t)Y2 * nx1 + X2)};
}
__device__ __forceinline__ float glare_up(const GlareUp& t, uint32_t ch) {
    return (0.5625f * t.e00[ch] + 0.1875f * t.e10[ch]) + (0.1875f * t.e01[ch] + 0.0625f * t.e11[ch]);
}

// u [nx x rows] = w d + U(u1), u1 [nx1 x rows1] the level above; u1 NULL (the coarsest level): u = w d
__global__ __launch_bounds__(256) void k_glare_up(const float* __restrict__ d, const float* __restrict__ u1, float* __restrict__ u, float w, uint32_t nx,
                                                  uint32_t rows, uint32_t nx1, uint32_t rows1) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx * rows) return;
    if (!u1) {
        for (uint32_t ch = 0; ch < 3u; ++ch) u[3 * (size_t)p + ch] = w * d[3 * (size_t)p + ch];
        return;
    }
    const GlareUp t = glare_up_taps(u1, p % nx, p / nx, nx1, rows1);
    for (uint32_t ch = 0; ch < 3u; ++ch) u[3 * (size_t)p + ch] = w * d[3 * (size_t)p + ch] + glare_up(t, ch);
}

// out [nx x rows] from c and u1 [nx1 x rows1]; u1 NULL (Le = 0, a 1 x 1 frame): out = s.  A pixel with a non-finite channel: out = c.
__global__ __launch_bounds__(256) void k_glare_combine(const float* __restrict__ c, const float* __restrict__ u1, float* __restrict__ out, uint32_t nx,
                                                       uint32_t rows, uint32_t nx1, uint32_t rows1, float amount, float threshold) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx * rows) return;
    float s[3], b[3], raw[3];
    const bool fin = glare_bright(c, p, threshold, s, b, raw);
    float o[3];
    if (!fin) {
        for (int ch = 0; ch < 3; ++ch) o[ch] = raw[ch];
    } else if (!u1) {
        for (int ch = 0; ch < 3; ++ch) o[ch] = s[ch];
    } else {
        const GlareUp t = glare_up_taps(u1, p % nx, p / nx, nx1, rows1);
        for (uint32_t ch = 0; ch < 3u; ++ch) o[ch] = (s[ch] - amount * b[ch]) + amount * glare_up(t, ch);
    }
    for (uint32_t ch = 0; ch < 3u; ++ch) out[3 * (size_t)p + ch] = o[ch];
}

} // namespace rt
