// rt_display.h — the kernels of "Display transform" (rtow_mi355x.h): the last stage of an accumulation's 8-bit output.  Three kernels over
// an f32 image in the call's row order, on the context's stream, no host decision in between:
//   k_display_stats    : one pass — per workgroup an LDS histogram of bits(Y) >> 20 (flushed to the global one by integer atomics on the
//                        non-zero bins), per 256 pixels the f64 partial sum of log Y on the tree of k_noise_partials, and the lit count;
//   k_display_exposure : ONE workgroup — the partials in index order (the tree of k_noise_final) or the scan of the 2048 bins, then e and
//                        the figures into the RtDisplayInfo record in device memory;
//   k_display          : exposure, curve, transfer, dither, quantisation and flip per pixel; e comes from that record; the saturated and
//                        the non-finite counts leave by one integer atomic per wave where the count is not zero.
// The counts go to RT_DISPLAY_SLOTS counters, a workgroup's to slot blockIdx & 255, and are added up by whoever reads them: on a bright
// frame every wave has saturated values, and 130 000 atomics on ONE word took 1.5 ms of a 3840 x 2160 k_display that takes 0.17 ms.
// A manual exposure launches k_display alone.  No floating-point atomic anywhere: every figure is the same bits on every run.
// Every f32 operation is one IEEE operation in the header's order (-ffp-contract=off).  GPU-free parts: rt_display_plan.h.
#pragma once
#include "rt_display_plan.h"
#include "rt_kernels.h"

namespace rt {

constexpr uint32_t RT_DISPLAY_GROUPS = 16u; // 256-pixel groups per workgroup of k_display_stats: one LDS histogram serves 4096 pixels
constexpr uint32_t RT_DISPLAY_SLOTS = 256u;
struct DisplayCounters { // one slot: zeroed before the kernels run
    unsigned long long n_lit, n_non_finite, n_saturated, reserved;
};

// The record k_display_exposure writes is the caller's RtDisplayInfo; its two last counts are the slots', added up by the host.
static_assert(sizeof(RtDisplayInfo) == 40u, "RtDisplayInfo: f32 x 2, f64, u64 x 3");

__device__ __forceinline__ float display_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ bool display_finite(float x) { return fabsf(x) <= RT_FLT_MAX; } // (a NaN compares false)

// `partials`: one f64 per 256-pixel group (want_log); `hist`: RT_DISPLAY_BINS u32, zeroed (want_hist); slots: zeroed.
__global__ __launch_bounds__(256) void k_display_stats(const float* __restrict__ img, uint32_t npix, uint32_t n_groups, uint32_t want_hist, uint32_t want_log,
                                                       uint32_t* __restrict__ hist, double* __restrict__ partials, DisplayCounters* __restrict__ slots) {
    __shared__ uint32_t s_hist[RT_DISPLAY_BINS];
    __shared__ double2 part[4];
    __shared__ uint32_t s_lit;
    const uint32_t lane = threadIdx.x & 63u;
    if (want_hist)
        for (uint32_t k = threadIdx.x; k < RT_DISPLAY_BINS; k += 256u) s_hist[k] = 0u;
    if (threadIdx.x == 0u) s_lit = 0u;
    __syncthreads();
    uint32_t n_lit = 0u;
    for (uint32_t g = 0u; g < RT_DISPLAY_GROUPS; ++g) {
        const uint32_t grp = blockIdx.x * RT_DISPLAY_GROUPS + g;
        if (grp >= n_groups) break; // (the same for every thread of the workgroup)
        const uint32_t p = grp * 256u + threadIdx.x;
        float y = 0.0f;
        if (p < npix) y = display_luminance(img[3 * (size_t)p], img[3 * (size_t)p + 1], img[3 * (size_t)p + 2]);
        const bool lit = y > 0.0f && y <= RT_FLT_MAX; // (tail slots, NaN, inf and whatever is not positive: not lit)
        n_lit += lit ? 1u : 0u;
        if (want_hist) {
            // A flat region puts a whole wave into one bin: the lanes that share the first lit lane's bin add their count once; the
            // others add one each.  Integer additions: the order does not matter.
            const uint32_t bin = lit ? display_bin_of_bits(__float_as_uint(y)) : 0xFFFFFFFFu; // (lit: <= RT_DISPLAY_LAST_BIN)
            const unsigned long long lit_mask = __ballot(lit);
            if (lit_mask) {
                const int leader = __ffsll((long long)lit_mask) - 1;
                const uint32_t lead_bin = (uint32_t)__shfl((int)bin, leader);
                const unsigned long long same = __ballot(lit && bin == lead_bin);
                if ((int)lane == leader) atomicAdd(&s_hist[lead_bin], (uint32_t)__popcll(same));
                else if (lit && bin != lead_bin) atomicAdd(&s_hist[bin], 1u);
            }
        }
        if (want_log) {
            const double2 s = block_sum_256(lit ? log((double)y) : 0.0, 0.0, part);
            if (threadIdx.x == 0u) partials[grp] = s.x;
            __syncthreads(); // (`part` is written again by the next group)
        }
    }
    for (int off = 32; off > 0; off >>= 1) n_lit += __shfl_down(n_lit, off);
    if (lane == 0u && n_lit) atomicAdd(&s_lit, n_lit);
    __syncthreads();
    if (threadIdx.x == 0u && s_lit) atomicAdd(&slots[blockIdx.x & (RT_DISPLAY_SLOTS - 1u)].n_lit, (unsigned long long)s_lit);
    if (want_hist)
        for (uint32_t k = threadIdx.x; k < RT_DISPLAY_BINS; k += 256u) {
            const uint32_t v = s_hist[k];
            if (v) atomicAdd(&hist[k], v);
        }
}

// ONE workgroup.  RT_EXPOSURE_KEY: thread t adds the partials t, t + 256, .. in index order, then lanes and waves as block_sum_256 adds
// them; RT_EXPOSURE_PERCENTILE: thread t owns the bins 8 t .. 8 t + 7, an inclusive scan over the threads finds the one whose bins hold
// the rank.  n_lit is the sum of what k_display_stats counted into the slots.
__global__ __launch_bounds__(256) void k_display_exposure(const double* __restrict__ partials, uint32_t n_groups, const uint32_t* __restrict__ hist,
                                                          const DisplayCounters* __restrict__ slots, RtDisplay d, RtDisplayInfo* __restrict__ info) {
    __shared__ double2 part[4];
    __shared__ unsigned long long s_scan[256];
    __shared__ unsigned long long s_lit;
    __shared__ uint32_t s_bin;
    static_assert(RT_DISPLAY_SLOTS == 256u, "one slot per thread");
    if (threadIdx.x == 0u) s_lit = 0u;
    __syncthreads();
    if (const unsigned long long mine = slots[threadIdx.x].n_lit) atomicAdd(&s_lit, mine);
    __syncthreads();
    const unsigned long long n_lit = s_lit;
    if (threadIdx.x == 0u) info->n_lit = n_lit;
    if (d.exposure_mode == RT_EXPOSURE_KEY) {
        double a = 0.0;
#pragma unroll 8
        for (uint32_t k = threadIdx.x; k < n_groups; k += 256u) a += partials[k]; // (in index order; the loads may run ahead)
        const double2 s = block_sum_256(a, 0.0, part);
        if (threadIdx.x != 0u) return;
        const double lavg = n_lit ? exp(s.x / (double)n_lit) : 0.0;
        info->log_average = lavg;
        info->percentile_luminance = 0.0f;
        info->exposure = n_lit ? display_exposure(d.exposure_value, lavg) : 1.0f;
        return;
    }
    uint32_t c[8];
    unsigned long long mine = 0u;
    for (uint32_t j = 0u; j < 8u; ++j) c[j] = hist[8u * threadIdx.x + j], mine += c[j];
    s_scan[threadIdx.x] = mine;
    if (threadIdx.x == 0u) s_bin = RT_DISPLAY_BINS;
    __syncthreads();
    for (uint32_t off = 1u; off < 256u; off <<= 1) {
        const unsigned long long v = threadIdx.x >= off ? s_scan[threadIdx.x - off] : 0u;
        __syncthreads();
        s_scan[threadIdx.x] += v;
        __syncthreads();
    }
    const unsigned long long rank = display_rank(d.percentile, n_lit), incl = s_scan[threadIdx.x];
    unsigned long long cum = incl - mine;
    if (n_lit && cum < rank && rank <= incl) // (exactly one thread: the cumulative counts do not decrease)
        for (uint32_t j = 0u; j < 8u; ++j) {
            cum += c[j];
            if (cum >= rank) {
                s_bin = 8u * threadIdx.x + j;
                break;
            }
        }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    const uint32_t b = s_bin;
    const float lq = b < RT_DISPLAY_BINS ? __uint_as_float(display_bin_mid_bits(b)) : 0.0f;
    info->log_average = 0.0;
    info->percentile_luminance = lq;
    info->exposure = b < RT_DISPLAY_BINS ? display_exposure(d.exposure_value, (double)lq) : 1.0f;
}

// One channel from the curve's output t to its 8-bit level: transfer, quantisation with the pixel's dither offset, k_finalize's rule.
__device__ __forceinline__ uint32_t display_level(float t, uint32_t transfer, bool dither, float offset) {
    float y;
    if (transfer == RT_TRANSFER_SRGB) y = t <= 0.0031308f ? 12.92f * t : 1.055f * (float)pow((double)t, 1.0 / 2.4) - 0.055f;
    else y = sqrtf(t);
    const float g = dither ? y * 255.0f + offset : y * 255.99f;
    return (g == g && g > 0.0f) ? (g >= 255.0f ? 255u : (uint32_t)g) : 0u;
}

// img: f32 x 3 per pixel in the call's row order; out_u8: rows flipped, as k_finalize writes them.  e: e_src->exposure where e_src is
// given (k_display_exposure wrote it), else d.exposure_value (manual).  slots: n_saturated and n_non_finite zeroed before.
__global__ __launch_bounds__(256) void k_display(const float* __restrict__ img, uint8_t* __restrict__ out_u8, uint32_t nx, uint32_t rows, RtDisplay d,
                                                 const RtDisplayInfo* __restrict__ e_src, DisplayCounters* __restrict__ slots) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const float e = e_src ? e_src->exposure : d.exposure_value;
    uint32_t n_sat = 0u;
    bool bad = false;
    if (p < nx * rows) {
        const uint32_t lj = p / nx, i = p - lj * nx, r = rows - 1u - lj; // (column and row of out_rgb8, row 0 on top)
        const float c[3] = {img[3 * (size_t)p], img[3 * (size_t)p + 1], img[3 * (size_t)p + 2]};
        const bool fin[3] = {display_finite(c[0]), display_finite(c[1]), display_finite(c[2])};
        bad = !(fin[0] && fin[1] && fin[2]);
        float t[3];
        for (int k = 0; k < 3; ++k) {
            const float x = e * c[k];
            t[k] = x > 0.0f ? x : 0.0f;
        }
        if (!bad && d.curve == RT_TONE_REINHARD) {
            const float L = display_luminance(t[0], t[1], t[2]);
            const float s = (1.0f + L / (d.white * d.white)) / (1.0f + L);
            for (int k = 0; k < 3; ++k) t[k] = t[k] * s;
        } else if (!bad && d.curve == RT_TONE_ACES) {
            for (int k = 0; k < 3; ++k) {
                const float x = t[k] < 65536.0f ? t[k] : 65536.0f;
                t[k] = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
            }
        }
        const bool dither = d.dither == RT_DITHER_BAYER8;
        const float offset = dither ? ((float)display_bayer(i & 7u, r & 7u) + 0.5f) / 64.0f : 0.0f;
        const size_t dst = ((size_t)r * nx + i) * 3u;
        for (int k = 0; k < 3; ++k) {
            uint32_t u;
            if (fin[k]) u = display_level(t[k], d.transfer, dither, offset);
            else u = c[k] > 0.0f ? 255u : 0u; // (+inf: 255; -inf and NaN: 0)
            n_sat += u == 255u ? 1u : 0u;
            out_u8[dst + k] = (uint8_t)u;
        }
    }
    const uint32_t n_bad = (uint32_t)__popcll(__ballot(bad));
    for (int off = 32; off > 0; off >>= 1) n_sat += __shfl_down(n_sat, off);
    if ((threadIdx.x & 63u) == 0u) {
        DisplayCounters* slot = slots + (blockIdx.x & (RT_DISPLAY_SLOTS - 1u));
        if (n_sat) atomicAdd(&slot->n_saturated, (unsigned long long)n_sat);
        if (n_bad) atomicAdd(&slot->n_non_finite, (unsigned long long)n_bad);
    }
}

} // namespace rt
