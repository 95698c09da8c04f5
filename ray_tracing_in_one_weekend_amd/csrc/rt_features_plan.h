// rt_features_plan.h — the GPU-free arithmetic of "First-hit features" (rtow_mi355x.h): what makes an RtFeatures valid, which samples of a
// window contribute under a stride, how the 64 B record of a pixel lies in the accumulation's buffer, and what makes an RtAccumFeatures well
// formed (rt_accum_features_check).  Like rt_filter_plan.h: no context, no device call, plain values in and out;
// tests/features_plan_main.cpp runs it under AddressSanitizer + UBSan without a GPU.
#pragma once
#include "../../include/rtow_mi355x.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace rt {

// NULL: `f` is what rt_accum_track_features accepts.  Else: what is wrong with it.
inline const char* features_invalid(const RtFeatures* f) {
    if (!f) return "the RtFeatures is NULL";
    if (f->stride < RT_FEATURES_MIN_STRIDE || f->stride > RT_FEATURES_MAX_STRIDE) return "stride must be RT_FEATURES_MIN_STRIDE .. RT_FEATURES_MAX_STRIDE";
    if (f->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

// Sample s (absolute index) takes a feature sample iff s % stride == 0.  The first such index at or behind i0 (64 bit: it may lie past 2^32).
inline uint64_t features_first(uint64_t i0, uint32_t stride) { return (i0 + stride - 1u) / stride * stride; }
// How many of the samples i0 .. i0 + n - 1 contribute (stride >= 1).
inline uint32_t features_in_window(uint32_t i0, uint32_t n, uint32_t stride) {
    const uint64_t first = features_first(i0, stride), end = (uint64_t)i0 + n;
    return first < end ? (uint32_t)((end - 1u - first) / stride) + 1u : 0u;
}

// ---- the record ---------------------------------------------------------------------------------------------------------------------------
// RtFeaturePixel, 64 B, is four 16 B quarters: (albedo, n_f), (normal, n_h), (a2, n2), (z1, z2).  The accumulation keeps quarter k of local
// pixel lp at byte (k * npix + lp) * 16 of its buffer — four planes, so that a wave reads and writes 1 KiB contiguous per quarter — and a
// snapshot carries the records whole, in image order: to a PlaneTable (rt_accum_planes.h) that is ONE row of 16 B elements in 4 parts.
constexpr uint32_t RT_FEATURES_QUARTER_BYTES = 16u, RT_FEATURES_QUARTERS = 4u;
constexpr size_t RT_FEATURES_PIXEL_BYTES = (size_t)RT_FEATURES_QUARTER_BYTES * RT_FEATURES_QUARTERS;
static_assert(sizeof(RtFeaturePixel) == RT_FEATURES_PIXEL_BYTES, "RtFeaturePixel is four 16 B quarters");
static_assert(offsetof(RtFeaturePixel, n_f) == 12u && offsetof(RtFeaturePixel, normal) == 16u && offsetof(RtFeaturePixel, n_h) == 28u &&
                  offsetof(RtFeaturePixel, a2) == 32u && offsetof(RtFeaturePixel, z1) == 48u,
              "the quarters of RtFeaturePixel");
inline size_t features_buffer_bytes(uint64_t npix) { return (size_t)npix * RT_FEATURES_PIXEL_BYTES; }
inline size_t features_quarter_offset(uint64_t npix, uint32_t quarter) { return (size_t)npix * RT_FEATURES_QUARTER_BYTES * quarter; }
// What rt_accum_read_features stages per pixel, image order: albedo 3, normal 3, depth 1, hit 1, var 3 floats.
constexpr uint32_t RT_FEATURES_READ_FLOATS = 11u;
inline size_t features_read_bytes(uint64_t npix) { return (size_t)npix * RT_FEATURES_READ_FLOATS * sizeof(float); }

// NULL: `fs` is what rt_accum_import_features accepts before it compares it with an accumulation.  Else: what is wrong with it.  The plane
// is not read: values are not judged.
inline const char* accum_features_invalid(const RtAccumFeatures* fs) {
    if (!fs) return "the RtAccumFeatures is NULL";
    if (fs->reserved[0] != 0u || fs->reserved[1] != 0u) return "reserved must be 0";
    if (!fs->plane) return "plane must not be NULL";
    if ((uint64_t)fs->first_sample + fs->done > 0xFFFFFFFFull) return "first_sample + done must stay below 2^32, as RtParams.spp does";
    return features_invalid(&fs->features);
}

// NULL: `g` is what rt_accum_denoise_features accepts.  Else: what is wrong with it.
inline const char* feature_guide_invalid(const RtFeatureGuide* g) {
    if (!g) return "the RtFeatureGuide is NULL";
    for (const float k : {g->k_albedo, g->k_normal, g->k_depth})
        if (!std::isfinite(k) || !(k > 0.0f)) return "k_albedo, k_normal and k_depth must be finite and > 0";
    for (const float t : {g->tau_albedo, g->tau_normal, g->tau_depth})
        if (!std::isfinite(t) || !(t >= 0.0f)) return "tau_albedo, tau_normal and tau_depth must be finite and >= 0";
    if (g->use_mask & ~(RT_FEATURE_USE_ALBEDO | RT_FEATURE_USE_NORMAL | RT_FEATURE_USE_DEPTH)) return "use_mask holds a bit that is no RT_FEATURE_USE_*";
    if (g->reserved[0] != 0u || g->reserved[1] != 0u) return "reserved must be 0";
    return nullptr;
}
// What the filter reads per pixel beside (c, y, v), image order: 7 means (abar, nbar, zbar) and 3 variances of the mean (va, vn, vz).
constexpr uint32_t RT_FEATURES_MEAN_FLOATS = 7u, RT_FEATURES_VAR_FLOATS = 3u;
inline size_t features_guide_bytes(uint64_t npix) { return (size_t)npix * (RT_FEATURES_MEAN_FLOATS + RT_FEATURES_VAR_FLOATS) * sizeof(float); }

} // namespace rt
