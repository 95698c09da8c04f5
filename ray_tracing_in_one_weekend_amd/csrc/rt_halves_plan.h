// rt_halves_plan.h — the GPU-free arithmetic of "Half buffers" (rtow_mi355x.h): how many of a pixel's samples fall into each half, and
// what makes an RtAccumHalves well formed (rt_accum_halves_check).  The kernels of rt_halves.h call halves_count below, so the device and
// the host count with the same operations.  Like rt_adaptive_plan.h: no context, no device call, plain values in and out;
// tests/halves_plan_main.cpp runs it under AddressSanitizer + UBSan without a GPU.
#pragma once
#include "../../include/rtow_mi355x.h"

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RT_HALVES_HD __host__ __device__
#else
#define RT_HALVES_HD
#endif

namespace rt {

// n_h: the number of absolute sample indices i in [first_sample, first_sample + n) with i & 1 == h.  Half 0 takes the even ones:
// floor(n / 2) of them and, where n is odd and the window starts on an even index, one more.  No sum of the arguments is formed, so
// nothing wraps at n = 2^32 - 1.
RT_HALVES_HD inline uint32_t halves_count(uint32_t first_sample, uint32_t n, uint32_t h) {
    const uint32_t even = (n >> 1) + (n & 1u & ~first_sample);
    return h ? n - even : even;
}

// NULL: `hs` is what rt_accum_import_halves accepts before it compares it with an accumulation.  Else: what is wrong with it.  No plane is
// read: values are not judged.
inline const char* accum_halves_invalid(const RtAccumHalves* hs) {
    if (!hs) return "the RtAccumHalves is NULL";
    if (hs->reserved[0] != 0u || hs->reserved[1] != 0u) return "reserved must be 0";
    if (!hs->sum[0] || !hs->sum[1] || !hs->moments[0] || !hs->moments[1]) return "sum[0], sum[1], moments[0] and moments[1] must not be NULL";
    if ((uint64_t)hs->first_sample + hs->done > 0xFFFFFFFFull) return "first_sample + done must stay below 2^32, as RtParams.spp does";
    return nullptr;
}

// ---- byte sizes ---------------------------------------------------------------------------------------------------------------------------
constexpr size_t RT_HALVES_SUM_BYTES = 3 * sizeof(float), RT_HALVES_MOMENT_BYTES = 2 * sizeof(double);
// Bytes per pixel that tracking adds to an accumulation, and that a state of halves takes on the host: two halves of a sum and a moment pair.
constexpr size_t RT_HALVES_PIXEL_BYTES = 2 * (RT_HALVES_SUM_BYTES + RT_HALVES_MOMENT_BYTES);

// Where the four planes of npix pixels lie in one buffer: the 16 B aligned moments first (half 0, half 1), the sums behind them.  The
// accumulation's own buffer (local pixel order) and the staging buffer of a state (image order) share this layout.
struct HalvesLayout {
    size_t moments[2], sum[2], total;
};
inline HalvesLayout halves_layout(uint64_t npix) {
    HalvesLayout l{};
    size_t off = 0;
    for (int h = 0; h < 2; ++h) l.moments[h] = off, off += (size_t)npix * RT_HALVES_MOMENT_BYTES;
    for (int h = 0; h < 2; ++h) l.sum[h] = off, off += (size_t)npix * RT_HALVES_SUM_BYTES;
    l.total = off;
    return l;
}

} // namespace rt
