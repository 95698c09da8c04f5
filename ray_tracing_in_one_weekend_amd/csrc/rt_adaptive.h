// rt_adaptive.h — per-pixel adaptive sampling on top of an accumulation (rtow_mi355x.h "Adaptive sampling"): new kernels only.
//
//   k_adaptive_begin            : n_p = the samples every pixel holds so far, no pixel converged (the first adaptive add)
//   k_adaptive_decide<DECIDE>   : the criterion per pixel (sticky flag) and the integer partial sums of RtAdaptiveInfo per workgroup;
//                                 DECIDE false: only the sums (rt_accum_read_counts after the samples were added)
//   k_adaptive_info             : one workgroup over the partial sums
//   k_gen_primary_active<LENS>  : k_gen_primary for the pixels still active: the depth-0 queue holds their rays only, compacted
// What an adaptive accumulation shares with a uniform one is one kernel with a template flag, beside its uniform form:
// k_resolve_moments<true> (the active pixels; n_p += s_count) and the readers k_finalize<true>, k_sem<true>, k_noise_partials<true>,
// k_noise_final<true> (rt_kernels.h) and k_denoise_inputs<true> (rt_denoise.h), with the pixel's own n_p in the place of the one n.
//
// Nothing downstream of depth 0's materialised queue changes: a ray's identity is the slot in its record (qa.w), its key and its
// radiance slot follow from the slot (path_key_of_slot, rad_store), and every kernel reads `counts[shard]` rays from the front of a
// shard.  Which position of its shard a ray takes is therefore free — here it depends on the order in which workgroups arrive at the
// shard's counter — and no bit of any pixel depends on it.  The slots of converged pixels are never written, read or resolved.
#pragma once
#include "rt_adaptive_plan.h"
#include "rt_denoise.h"

namespace rt {

__global__ __launch_bounds__(256) void k_adaptive_begin(uint32_t* __restrict__ cnt, uint8_t* __restrict__ flag, uint32_t npix, uint32_t n) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npix) return;
    cnt[p] = n;
    flag[p] = 0u;
}

// The integer sums are AdaptiveSums (rt_kernels.h, beside k_noise_final, which reads the frame's spp_min).
// The fixed tree of block_sum_256 over integers: lanes by __shfl_down, the four waves through LDS in wave order.  (Integer sums do not
// depend on their order; the tree spares the atomics.)  Every thread of the workgroup calls it; thread 0 holds the result.
__device__ __forceinline__ AdaptiveSums adaptive_block_sums(AdaptiveSums s, AdaptiveSums* part) {
    for (int off = 32; off > 0; off >>= 1) {
        s.n_active += __shfl_down(s.n_active, off);
        s.n_samples += __shfl_down(s.n_samples, off);
        s.spp_min = min(s.spp_min, (uint32_t)__shfl_down((int)s.spp_min, off));
        s.spp_max = max(s.spp_max, (uint32_t)__shfl_down((int)s.spp_max, off));
    }
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    AdaptiveSums r = part[0];
    for (int k = 1; k < 4; ++k) {
        r.n_active += part[k].n_active, r.n_samples += part[k].n_samples;
        r.spp_min = min(r.spp_min, part[k].spp_min), r.spp_max = max(r.spp_max, part[k].spp_max);
    }
    return r;
}

// One lane per pixel, in the local pixel order of the accumulation.  DECIDE: a pixel that is still active and meets the criterion on the
// moments of its n_p samples becomes converged, for good.  Either way the workgroup's sums go to partials[blockIdx.x].
template <bool DECIDE>
__global__ __launch_bounds__(256) void k_adaptive_decide(const double2* __restrict__ mom, const uint32_t* __restrict__ cnt, uint8_t* __restrict__ flag,
                                                         AdaptiveSums* __restrict__ partials, uint32_t npix, double tolerance, double luminance_floor,
                                                         uint32_t min_samples) {
    __shared__ AdaptiveSums part[4];
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    AdaptiveSums s{0ull, 0ull, 0xFFFFFFFFu, 0u}; // (tail lanes contribute nothing)
    if (p < npix) {
        const uint32_t n = cnt[p];
        bool conv = flag[p] != 0u;
        if (DECIDE && !conv) {
            double ybar, v;
            pixel_noise(mom[p], n, ybar, v);
            conv = adaptive_converged(ybar, v, n, tolerance, luminance_floor, min_samples);
            if (conv) flag[p] = 1u;
        }
        s = AdaptiveSums{conv ? 0ull : 1ull, (unsigned long long)n, n, n};
    }
    const AdaptiveSums r = adaptive_block_sums(s, part);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}
// ONE workgroup over the partial sums, thread t taking partials t, t + 256, ...
__global__ __launch_bounds__(256) void k_adaptive_info(const AdaptiveSums* __restrict__ partials, uint32_t n_partials, AdaptiveSums* __restrict__ out) {
    __shared__ AdaptiveSums part[4];
    AdaptiveSums s{0ull, 0ull, 0xFFFFFFFFu, 0u};
    for (uint32_t k = threadIdx.x; k < n_partials; k += 256u) {
        const AdaptiveSums q = partials[k];
        s.n_active += q.n_active, s.n_samples += q.n_samples;
        s.spp_min = min(s.spp_min, q.spp_min), s.spp_max = max(s.spp_max, q.spp_max);
    }
    const AdaptiveSums r = adaptive_block_sums(s, part);
    if (threadIdx.x == 0) *out = r;
}

// The primary rays of the active pixels of a slice.  A workgroup is one chunk of 256 consecutive slots, its shard chunk % nq as in
// k_gen_primary.  A lane whose pixel has converged does nothing past its flag load (it stays for the two barriers).  The active lanes
// are ranked by ballot / mbcnt within their wave, the four wave totals meet in LDS, and ONE atomic add per workgroup on counts[shard]
// claims the chunk's span in the shard: records at shard * cap + base + rank, slot = idx, T = 1.  A shard takes at most 256 rays from
// each of its chunks, so its count stays within shard_cap (rt_frame_plan.h) like the closed form of k_init_counts.  `counts` (depth 0,
// [nq]) is cleared before the launch and is what every depth-0 kernel then reads.
template <bool LENS>
__global__ __launch_bounds__(256) void k_gen_primary_active(GenParams gp, Queue q, GenLens gl, const uint8_t* __restrict__ flag,
                                                            uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_base;
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    bool active = false;
    if (idx < gp.n_rays) {
        uint32_t pl;
        (void)udiv_inv(idx, gp.npix, gp.inv_npix, pl); // pl = local pixel, as gen_primary finds it
        active = flag[pl] == 0u;
    }
    const unsigned long long m = __ballot(active);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) s_wave[w] = (uint32_t)__popcll(m);
    __syncthreads();
    const uint32_t sq = blockIdx.x % gp.nq;
    if (threadIdx.x == 0) {
        const uint32_t total = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        s_base = total ? atomicAdd(&counts[sq], total) : 0u;
    }
    __syncthreads();
    if (!active) return;
    uint32_t off = s_base + rank;
    for (uint32_t k = 0; k < w; ++k) off += s_wave[k];
    V3 o, d;
    uint32_t k0, k1;
    gen_primary<LENS>(gp, gl, idx, o, d, k0, k1);
    const size_t pos = (size_t)sq * gp.cap + off;
    q.a[RT_QSTRIDE * pos] = make_float4(o.x, o.y, o.z, __uint_as_float(idx));
    q.b[RT_QSTRIDE * pos] = make_float4(d.x, d.y, d.z, 1.0f);
    q.c[pos] = make_float2(1.0f, 1.0f);
}

} // namespace rt
