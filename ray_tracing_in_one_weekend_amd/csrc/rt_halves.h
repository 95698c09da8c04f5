// rt_halves.h — the two half buffers of an accumulation, the cross-filtered denoise and its residual (rtow_mi355x.h "Half buffers"): new
// kernels only; no kernel of rt_kernels.h, rt_adaptive.h, rt_denoise.h, rt_channels.h or rt_accum_state_kernels.h changes, and none of
// these is in a variant table or a ledger family.
//
//   k_resolve_halves<ACTIVE>        : the slice's samples onto the half sums and moments by the parity of their absolute index
//   k_halves_read<COUNTS>           : one half as an image and its standard error, in image order
//   k_denoise_inputs_halves<COUNTS> : c_0, c_1, (y, v)_0, (y, v)_1 in image order — what the two launches of k_denoise<F> read (rt_denoise.h:
//                                     nlm_filter with one guide plane), each half by the other's (y, v)
//   k_halves_combine<COUNTS>        : out and e per pixel from f_0 and f_1, and the per-workgroup partial sums of the frame figures
//   k_halves_final                  : one workgroup over the partials -> mean_luminance, residual_rms, residual_noise
// (rt_accum_export_halves and _import_halves move the four planes as a PlaneTable through k_planes_move, rt_accum_state_kernels.h.)
//
// HalfPlanes in the accumulation's local pixel order: per half a plane of RGB triples and a plane of double2 (S1, S2).  A lane reads and
// writes 12 B at stride 12 B and 16 B at stride 16 B per plane, as k_resolve_moments does on the whole-pixel sums.  COUNTS: the pixel's own
// n_p (an adaptive accumulation); n_h follows from (first_sample, n_p) by halves_count and is stored nowhere.
#pragma once
#include "rt_accum_state_kernels.h"
#include "rt_halves_plan.h"

namespace rt {

struct HalfPlanes {
    float* sum[2];     // [npix * 3]
    double2* mom[2];   // [npix]
};

// One sample of one half: the arithmetic of k_resolve_moments.
struct HalfSums {
    StateRgb c;
    double2 m;
};
__device__ __forceinline__ void half_sums_add(HalfSums& a, float sx, float sy, float sz) {
    a.c.r += sx;
    a.c.g += sy;
    a.c.b += sz;
    const double y = sample_luminance(sx, sy, sz);
    a.m.x += y;
    a.m.y += y * y;
}

// i0: the absolute index of the slice's first sample.  Sample s of the slice has the parity of i0 + s: the half of i0's parity takes
// s = 0, 2, 4, .., the other one s = 1, 3, .., each in sample order.  So the loop goes in pairs on two fixed sets of registers (no half is
// picked per sample), and the two loads of a pair are issued before the first of their additions.  ACTIVE: converged pixels are skipped —
// nothing wrote their radiance slots; the active ones all hold the same number of samples, hence the one i0.
template <bool ACTIVE>
__global__ __launch_bounds__(256) void k_resolve_halves(const float* __restrict__ rad, HalfPlanes hp, const uint8_t* __restrict__ flag, uint32_t npix,
                                                        uint32_t i0, uint32_t s_count) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npix) return;
    if (ACTIVE && flag[p] != 0u) return;
    const uint32_t ha = i0 & 1u, hb = ha ^ 1u;
    HalfSums a, b;
    a.c = reinterpret_cast<const StateRgb*>(hp.sum[ha])[p], a.m = hp.mom[ha][p];
    b.c = reinterpret_cast<const StateRgb*>(hp.sum[hb])[p], b.m = hp.mom[hb][p];
    const size_t stride = (size_t)RT_RAD_FLOATS * npix;
    const float* src = rad + RT_RAD_FLOATS * (size_t)p;
    uint32_t s = 0;
    for (; s + 2u <= s_count; s += 2u, src += 2 * stride) {
        const float* s1 = src + stride;
        const float x0 = src[0], y0 = src[1], z0 = src[2];
        const float x1 = s1[0], y1 = s1[1], z1 = s1[2];
        half_sums_add(a, x0, y0, z0);
        half_sums_add(b, x1, y1, z1);
    }
    if (s < s_count) half_sums_add(a, src[0], src[1], src[2]);
    reinterpret_cast<StateRgb*>(hp.sum[ha])[p] = a.c, hp.mom[ha][p] = a.m;
    if (s_count >= 2u) reinterpret_cast<StateRgb*>(hp.sum[hb])[p] = b.c, hp.mom[hb][p] = b.m;
}

// What a reader needs of one pixel: its local index and the sample counts of its halves.
struct HalfPixel {
    size_t ap;
    uint32_t n[2];
};
template <bool COUNTS>
__device__ __forceinline__ HalfPixel half_pixel(const uint32_t* __restrict__ cnt, uint32_t p, uint32_t nx, uint32_t first, uint32_t n, uint32_t tiles_per_row,
                                                uint32_t tile_pixels) {
    HalfPixel hx;
    hx.ap = local_of_pixel(nx, tiles_per_row, tile_pixels, p % nx, p / nx);
    if (COUNTS) n = cnt[hx.ap];
    hx.n[0] = halves_count(first, n, 0u);
    hx.n[1] = n - hx.n[0];
    return hx;
}
__device__ __forceinline__ StateRgb half_colour(const float* __restrict__ sum, size_t ap, uint32_t n) {
    const float fs = (float)(n ? n : 1u);
    const StateRgb s = reinterpret_cast<const StateRgb*>(sum)[ap];
    return StateRgb{s.r / fs, s.g / fs, s.b / fs};
}

// rt_accum_read_halves: sum_h / (float)max(n_h, 1) and (float)sqrt(V_h) (pixel_noise: 0 where n_h < 2), in image order; either output may be NULL.
template <bool COUNTS>
__global__ __launch_bounds__(256) void k_halves_read(HalfPlanes hp, const uint32_t* __restrict__ cnt, uint32_t h, float* __restrict__ out_rgb,
                                                     float* __restrict__ out_sem, uint32_t nx, uint32_t rows, uint32_t first, uint32_t n,
                                                     uint32_t tiles_per_row, uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx * rows) return;
    const HalfPixel hx = half_pixel<COUNTS>(cnt, p, nx, first, n, tiles_per_row, tile_pixels);
    const uint32_t nh = h ? hx.n[1] : hx.n[0];
    if (out_rgb) reinterpret_cast<StateRgb*>(out_rgb)[p] = half_colour(h ? hp.sum[1] : hp.sum[0], hx.ap, nh);
    if (out_sem) {
        double ybar, v;
        pixel_noise((h ? hp.mom[1] : hp.mom[0])[hx.ap], nh, ybar, v);
        out_sem[p] = (float)sqrt(v);
    }
}

// The inputs of the two filter launches: per half c_h and (y_h, v_h) = ((float)Ybar_h, (float)V_h) with n = n_h, NaN where n_h < 2 as in
// k_denoise_inputs<true>: such a half pixel guides nobody and, as a guide of the other half, makes that pixel keep its own colour.
template <bool COUNTS>
__global__ __launch_bounds__(256) void k_denoise_inputs_halves(HalfPlanes hp, const uint32_t* __restrict__ cnt, float* __restrict__ c0, float* __restrict__ c1,
                                                               float2* __restrict__ yv0, float2* __restrict__ yv1, uint32_t nx, uint32_t rows,
                                                               uint32_t first, uint32_t n, uint32_t tiles_per_row, uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx * rows) return;
    const HalfPixel hx = half_pixel<COUNTS>(cnt, p, nx, first, n, tiles_per_row, tile_pixels);
    reinterpret_cast<StateRgb*>(c0)[p] = half_colour(hp.sum[0], hx.ap, hx.n[0]);
    reinterpret_cast<StateRgb*>(c1)[p] = half_colour(hp.sum[1], hx.ap, hx.n[1]);
    const float none = __uint_as_float(0x7FC00000u);
    double ybar, v;
    pixel_noise(hp.mom[0][hx.ap], hx.n[0], ybar, v);
    yv0[p] = hx.n[0] >= 2u ? make_float2((float)ybar, (float)v) : make_float2(none, none);
    pixel_noise(hp.mom[1][hx.ap], hx.n[1], ybar, v);
    yv1[p] = hx.n[1] >= 2u ? make_float2((float)ybar, (float)v) : make_float2(none, none);
}

// l(x) of the header: Rec. 709 luminance in f32, every operation one f32 operation in this order.
__device__ __forceinline__ float halves_luminance(StateRgb x) { return (0.2126f * x.r + 0.7152f * x.g) + 0.0722f * x.b; }
__device__ __forceinline__ float halves_mix(float f0, float f1, float a0, float a1) { return (f0 * a0 + f1 * a1) / (a0 + a1); }

// out = (f_0 a_0 + f_1 a_1) / (a_0 + a_1), a_h = (float)n_h (the half that holds samples where the other holds none);
// e = (d d) ((a_0 a_1) / ((a_0 + a_1)(a_0 + a_1))), d = l(f_0) - l(f_1), NaN where a half holds no sample.  partials[workgroup] =
// (sum (double)l(out), sum (double)e) over its 256 pixels by block_sum_256; tail slots contribute nothing.
template <bool COUNTS>
__global__ __launch_bounds__(256) void k_halves_combine(const float* __restrict__ f0, const float* __restrict__ f1, const uint32_t* __restrict__ cnt,
                                                        float* __restrict__ out, float* __restrict__ err, double2* __restrict__ partials, uint32_t nx,
                                                        uint32_t rows, uint32_t first, uint32_t n, uint32_t tiles_per_row, uint32_t tile_pixels) {
    __shared__ double2 part[4];
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    double lum = 0.0, e64 = 0.0;
    if (p < nx * rows) {
        const HalfPixel hx = half_pixel<COUNTS>(cnt, p, nx, first, n, tiles_per_row, tile_pixels);
        const StateRgb x0 = reinterpret_cast<const StateRgb*>(f0)[p], x1 = reinterpret_cast<const StateRgb*>(f1)[p];
        const float a0 = (float)hx.n[0], a1 = (float)hx.n[1];
        StateRgb o{halves_mix(x0.r, x1.r, a0, a1), halves_mix(x0.g, x1.g, a0, a1), halves_mix(x0.b, x1.b, a0, a1)};
        if (hx.n[1] == 0u) o = x0;
        else if (hx.n[0] == 0u) o = x1;
        const float d = halves_luminance(x0) - halves_luminance(x1);
        float e = (d * d) * ((a0 * a1) / ((a0 + a1) * (a0 + a1)));
        if (hx.n[0] == 0u || hx.n[1] == 0u) e = __uint_as_float(0x7FC00000u);
        reinterpret_cast<StateRgb*>(out)[p] = o;
        err[p] = e;
        lum = (double)halves_luminance(o), e64 = (double)e;
    }
    const double2 s = block_sum_256(lum, e64, part);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// out[0] = mean_luminance, out[1] = residual_rms, out[2] = residual_noise (RtResidual); the tree and the zero rule of k_noise_final.
__global__ __launch_bounds__(256) void k_halves_final(const double2* __restrict__ partials, uint32_t n_partials, uint32_t npix, double* __restrict__ out) {
    __shared__ double2 part[4];
    double a = 0.0, b = 0.0;
    for (uint32_t k = threadIdx.x; k < n_partials; k += 256u) a += partials[k].x, b += partials[k].y;
    const double2 s = block_sum_256(a, b, part);
    if (threadIdx.x != 0) return;
    const double mean = s.x / (double)npix, rms = sqrt(s.y / (double)npix);
    double noise = rms / mean;
    if (mean == 0.0) noise = rms == 0.0 ? 0.0 : (double)INFINITY;
    out[0] = mean, out[1] = rms, out[2] = noise;
}

} // namespace rt
