// rt_buckets_plan.h — the GPU-free arithmetic of "Sample buckets" (rtow_mi355x.h): how many of a pixel's samples fall into each bucket,
// what makes an RtAccumBuckets and an RtRobust well formed (rt_accum_buckets_check), and where the planes lie.  The kernels of
// rt_buckets.h call buckets_count below, so the device and the host count with the same operations.  Like rt_halves_plan.h: no context,
// no device call, plain values in and out; tests/buckets_plan_main.cpp runs it under AddressSanitizer + UBSan without a GPU.
#pragma once
#include "../../include/rtow_mi355x.h"

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RT_BUCKETS_HD __host__ __device__
#else
#define RT_BUCKETS_HD
#endif

namespace rt {

constexpr uint32_t RT_BUCKETS_MIN = 3u;
static_assert(sizeof(((RtAccumBuckets*)nullptr)->sum) / sizeof(float*) == RT_BUCKETS_MAX, "RtAccumBuckets.sum holds RT_BUCKETS_MAX planes");

// n_b: the number of absolute sample indices i in [first_sample, first_sample + n) with i % M == b, for 1 <= M and b < M.  The window
// holds n / M whole cycles, which give every bucket one sample each; the n % M samples that are left start at an index congruent to
// first_sample, so they go to the buckets first_sample % M, first_sample % M + 1, .. (mod M): bucket b gets one of them when its distance
// behind first_sample % M on that cycle is below n % M.  No sum of first_sample and n is formed, so nothing wraps at 2^32 - 1.
RT_BUCKETS_HD inline uint32_t buckets_count(uint32_t first_sample, uint32_t n, uint32_t M, uint32_t b) {
    const uint32_t q = n / M, r = n - q * M, f = first_sample % M;
    const uint32_t behind = b >= f ? b - f : b + (M - f);
    return q + (behind < r ? 1u : 0u);
}

// NULL: `bs` is what rt_accum_import_buckets accepts before it compares it with an accumulation.  Else: what is wrong with it.  No plane
// is read: values are not judged.  The pointers past M are not looked at.
inline const char* accum_buckets_invalid(const RtAccumBuckets* bs) {
    if (!bs) return "the RtAccumBuckets is NULL";
    if (bs->reserved != 0u) return "reserved must be 0";
    if (bs->M < RT_BUCKETS_MIN || bs->M > RT_BUCKETS_MAX) return "M must be 3 .. RT_BUCKETS_MAX";
    for (uint32_t b = 0; b < bs->M; ++b)
        if (!bs->sum[b]) return "sum[0] .. sum[M - 1] must not be NULL";
    if ((uint64_t)bs->first_sample + bs->done > 0xFFFFFFFFull) return "first_sample + done must stay below 2^32, as RtParams.spp does";
    return nullptr;
}

// NULL: `rb` (NULL: RT_ROBUST_GINI) is what the robust read-outs accept.  Else: what is wrong with it.
inline const char* robust_invalid(const RtRobust* rb) {
    if (!rb) return nullptr;
    if (rb->mode > RT_ROBUST_TRIM) return "mode must be RT_ROBUST_GINI, RT_ROBUST_MEDIAN or RT_ROBUST_TRIM";
    if (rb->reserved[0] != 0u || rb->reserved[1] != 0u) return "reserved must be 0";
    return nullptr;
}

// ---- byte sizes ---------------------------------------------------------------------------------------------------------------------------
constexpr size_t RT_BUCKETS_SUM_BYTES = 3 * sizeof(float);
// Bytes per pixel that tracking M buckets adds to an accumulation, and that a state of buckets takes on the host.
inline size_t buckets_pixel_bytes(uint32_t M) { return (size_t)M * RT_BUCKETS_SUM_BYTES; }
// Plane b of npix pixels begins buckets_plane(npix, b) bytes into the buffer: M planes of RGB triples, one behind the other.  The
// accumulation's own buffer (local pixel order) and the staging buffer of a state (image order) share this layout.
inline size_t buckets_plane(uint64_t npix, uint32_t b) { return (size_t)b * (size_t)npix * RT_BUCKETS_SUM_BYTES; }
inline size_t buckets_total(uint64_t npix, uint32_t M) { return buckets_plane(npix, M); }

} // namespace rt
