// rt_buckets.h — the M sample buckets of an accumulation and the median-of-means read-out (rtow_mi355x.h "Sample buckets"): new kernels
// only; no kernel of rt_kernels.h, rt_adaptive.h, rt_denoise.h, rt_channels.h, rt_accum_state_kernels.h or rt_halves.h changes, and none
// of these is in a variant table or a ledger family.
//
//   k_resolve_buckets<ACTIVE>          : the slice's samples onto the bucket sums by their absolute index modulo M
//   k_robust_read<COUNTS>              : the trimmed mean of the sorted bucket means per pixel and channel, its trim, and the per-workgroup
//                                        partial sums of the frame figures, in image order
//   k_robust_final                     : one workgroup over the partials -> RtRobustInfo
// (rt_accum_export_buckets and _import_buckets move the M planes as a PlaneTable through k_planes_move, rt_accum_state_kernels.h.)
//
// The planes lie one behind the other in one buffer (rt_buckets_plan.h), each npix RGB triples in the accumulation's local pixel order: a
// lane reads and writes 12 B at stride 12 B per plane, as k_resolve_moments does on the whole-pixel sums.  M is a run-time value
// everywhere; no kernel holds an array indexed by it in registers.
#pragma once
#include "rt_accum_state_kernels.h"
#include "rt_buckets_plan.h"

namespace rt {

// i0: the absolute index of the slice's first sample.  Sample s of the slice belongs to bucket (i0 + s) % M, so bucket (i0 + j) % M takes
// the samples j, j + M, j + 2M, .. in sample order: buckets on the outside — each sum is loaded once, kept in three registers and stored
// once — and its samples on the inside, the loads of the next one issued before the additions of this one.  Every radiance value of the
// slice is read exactly once.  ACTIVE: converged pixels are skipped — nothing wrote their radiance slots; the active ones all hold the
// same number of samples, hence the one i0.
template <bool ACTIVE>
__global__ __launch_bounds__(256) void k_resolve_buckets(const float* __restrict__ rad, float* __restrict__ buckets, const uint8_t* __restrict__ flag, uint32_t npix,
                                                         uint32_t M, uint32_t i0, uint32_t s_count) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npix) return;
    if (ACTIVE && flag[p] != 0u) return;
    const size_t stride = (size_t)RT_RAD_FLOATS * npix, plane = (size_t)3u * npix;
    const float* src0 = rad + RT_RAD_FLOATS * (size_t)p;
    const uint32_t nj = M < s_count ? M : s_count;
    uint32_t b = i0 % M;
    for (uint32_t j = 0; j < nj; ++j, src0 += stride) {
        StateRgb* slot = reinterpret_cast<StateRgb*>(buckets + (size_t)b * plane) + p;
        StateRgb a = *slot;
        const float* src = src0;
        float x = src[0], y = src[1], z = src[2];
        for (uint32_t s = j + M; s < s_count; s += M) {
            src += (size_t)M * stride;
            const float x1 = src[0], y1 = src[1], z1 = src[2];
            a.r += x, a.g += y, a.b += z;
            x = x1, y = y1, z = z1;
        }
        a.r += x, a.g += y, a.b += z;
        *slot = a;
        b = b + 1u == M ? 0u : b + 1u;
    }
}

// l(x) of "Half buffers": Rec. 709 luminance in f32, every operation one f32 operation in this order.
__device__ __forceinline__ float robust_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// The partial sums of one workgroup, and of the frame: f64 over the tree of block_sum_256, the integers exactly.
struct RobustPartial {
    double plain, robust;                  // sum (double)l(c_p), sum (double)l(out_p)
    unsigned long long trimmed, dropped;   // pixel-channels with t > 0; bucket means dropped as non-finite
};
// What k_robust_final writes: the fields of RtRobustInfo in their order.
struct RobustFigures {
    double mean_luminance_plain, mean_luminance_robust, energy_removed, trimmed_fraction;
    unsigned long long nonfinite_dropped;
};
static_assert(sizeof(RobustFigures) == sizeof(RtRobustInfo) && sizeof(RobustFigures) == 40u, "RobustFigures is RtRobustInfo");

__device__ __forceinline__ void block_count_256(unsigned long long& a, unsigned long long& b, unsigned long long* part) {
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off);
        b += __shfl_down(b, off);
    }
    if ((threadIdx.x & 63u) == 0) part[2u * (threadIdx.x >> 6)] = a, part[2u * (threadIdx.x >> 6) + 1u] = b;
    __syncthreads();
    a = part[0] + part[2] + part[4] + part[6];
    b = part[1] + part[3] + part[5] + part[7];
}

// One thread per pixel in image order.  Per channel, the finite bucket means go into the thread's own column of LDS — word i * 256 +
// threadIdx.x, so the 64 lanes of a wave touch 64 consecutive words whatever i is: no bank conflict and no barrier, nobody reads another
// thread's column — by an insertion sort, ascending; the sums of the header then walk the column in order.  16 KiB at RT_BUCKETS_MAX.
// out, out_trim: NULL or image order; `partials` NULL: no figures.  COUNTS: the pixel's own n_p.
template <bool COUNTS>
__global__ __launch_bounds__(256) void k_robust_read(const float* __restrict__ buckets, const float* __restrict__ sum, const uint32_t* __restrict__ cnt,
                                                     float* __restrict__ out, uint8_t* __restrict__ out_trim, RobustPartial* __restrict__ partials, uint32_t M,
                                                     uint32_t mode, uint32_t trim, uint32_t nx, uint32_t rows, uint32_t first, uint32_t n, uint32_t tiles_per_row,
                                                     uint32_t tile_pixels) {
    __shared__ float col[RT_BUCKETS_MAX * 256u];
    __shared__ double2 part[4];
    __shared__ unsigned long long ipart[8];
    const uint32_t p = blockIdx.x * 256u + threadIdx.x, npix = nx * rows;
    double lum_plain = 0.0, lum_robust = 0.0;
    unsigned long long trimmed = 0ull, dropped = 0ull;
    if (p < npix) {
        const size_t ap = local_of_pixel(nx, tiles_per_row, tile_pixels, p % nx, p / nx);
        if (COUNTS) n = cnt[ap];
        const size_t plane = (size_t)3u * npix;
        float* x = col + threadIdx.x;
        float o[3];
        for (uint32_t c = 0; c < 3u; ++c) {
            // 1. the finite means, sorted
            uint32_t K = 0;
            for (uint32_t b = 0; b < M; ++b) {
                const uint32_t nb = buckets_count(first, n, M, b);
                if (nb == 0u) continue;
                const float m = buckets[(size_t)b * plane + 3u * ap + c] / (float)nb;
                if (!(m - m == 0.0f)) {
                    ++dropped;
                    continue;
                }
                uint32_t i = K++;
                for (; i > 0u && x[(i - 1u) * 256u] > m; --i) x[i * 256u] = x[(i - 1u) * 256u];
                x[i * 256u] = m;
            }
            uint32_t t = 0;
            float res = __uint_as_float(0x7FC00000u);
            if (K > 0u) {
                const uint32_t tmax = (K - 1u) / 2u;
                if (mode == RT_ROBUST_MEDIAN) t = tmax;
                else if (mode == RT_ROBUST_TRIM) t = trim < tmax ? trim : tmax;
                else {
                    // 2. s and the rank-weighted w
                    float s = 0.0f, w = 0.0f;
                    for (uint32_t i = 0; i < K; ++i) {
                        const float xi = x[i * 256u];
                        s = s + xi;
                        w = w + (float)(i + 1u) * xi;
                    }
                    // 3. the normalised Gini coefficient of the means -> the trim
                    if (K >= 2u && s > 0.0f) {
                        const float fk = (float)K;
                        const float G = (2.0f * w) / (fk * s) - ((float)(K + 1u) / fk);
                        const float Gn = G * (fk / (float)(K - 1u));
                        if (Gn > 0.0f) {
                            const float h = (Gn * fk) * 0.5f; // (h >= 8 is beyond every tmax: the cast sees values it can hold only)
                            const uint32_t th = h >= 8.0f ? 8u : (uint32_t)h;
                            t = th < tmax ? th : tmax;
                        }
                    }
                }
                // 4. the trimmed mean
                float a = 0.0f;
                for (uint32_t i = t; i + t < K; ++i) a = a + x[i * 256u];
                res = a / (float)(K - 2u * t);
            }
            o[c] = res;
            if (out_trim) out_trim[3u * (size_t)p + c] = (uint8_t)t;
            trimmed += t > 0u ? 1ull : 0ull;
        }
        if (out) reinterpret_cast<StateRgb*>(out)[p] = StateRgb{o[0], o[1], o[2]};
        const float fs = (float)(n ? n : 1u);
        const StateRgb sp = reinterpret_cast<const StateRgb*>(sum)[ap];
        lum_plain = (double)robust_luminance(sp.r / fs, sp.g / fs, sp.b / fs);
        lum_robust = (double)robust_luminance(o[0], o[1], o[2]);
    }
    if (!partials) return; // (uniform over the grid: nobody waits at the barriers below)
    const double2 s = block_sum_256(lum_plain, lum_robust, part);
    block_count_256(trimmed, dropped, ipart);
    if (threadIdx.x == 0) partials[blockIdx.x] = RobustPartial{s.x, s.y, trimmed, dropped};
}

// One workgroup over the partials, thread t taking partials t, t + 256, .. in index order: the tree of k_noise_final.
__global__ __launch_bounds__(256) void k_robust_final(const RobustPartial* __restrict__ partials, uint32_t n_partials, uint32_t npix, RobustFigures* __restrict__ out) {
    __shared__ double2 part[4];
    __shared__ unsigned long long ipart[8];
    double a = 0.0, b = 0.0;
    unsigned long long trimmed = 0ull, dropped = 0ull;
    for (uint32_t k = threadIdx.x; k < n_partials; k += 256u) {
        a += partials[k].plain, b += partials[k].robust;
        trimmed += partials[k].trimmed, dropped += partials[k].dropped;
    }
    const double2 s = block_sum_256(a, b, part);
    block_count_256(trimmed, dropped, ipart);
    if (threadIdx.x != 0) return;
    const double plain = s.x / (double)npix, robust = s.y / (double)npix;
    double removed = 1.0 - robust / plain;
    if (plain == 0.0 && robust == 0.0) removed = 0.0;
    *out = RobustFigures{plain, robust, removed, (double)trimmed / (3.0 * (double)npix), dropped};
}

} // namespace rt
