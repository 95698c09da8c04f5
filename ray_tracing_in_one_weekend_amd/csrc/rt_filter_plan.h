// rt_filter_plan.h — the GPU-free arithmetic of "Pixel reconstruction filters" (rtow_mi355x.h): what makes an RtPixelFilter valid, the
// 256-entry table of its 1-D profile, its reach in pixels, and what makes an RtAccumFilter well formed (rt_accum_filter_check).  The
// kernels of rt_filter.h read the table and never evaluate a profile, so a host that holds the table can restate them bit for bit.  Like
// rt_halves_plan.h: no context, no device call, plain values in and out; tests/filter_plan_main.cpp runs it under AddressSanitizer + UBSan
// without a GPU.
#pragma once
#include "../../include/rtow_mi355x.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rt {

// NULL: `f` is a filter rt_accum_track_filter accepts.  Else: what is wrong with it.
inline const char* pixel_filter_invalid(const RtPixelFilter* f) {
    if (!f) return "the RtPixelFilter is NULL";
    if (f->kind > RT_FILTER_BLACKMAN_HARRIS) return "kind must be RT_FILTER_BOX .. RT_FILTER_BLACKMAN_HARRIS";
    if (!std::isfinite(f->radius) || !std::isfinite(f->p0) || !std::isfinite(f->p1)) return "radius, p0 and p1 must be finite";
    if (!(f->radius >= RT_FILTER_MIN_RADIUS && f->radius <= RT_FILTER_MAX_RADIUS)) return "radius must be RT_FILTER_MIN_RADIUS .. RT_FILTER_MAX_RADIUS";
    if (f->kind == RT_FILTER_GAUSSIAN && !(f->p0 > 0.0f)) return "the sigma of a Gaussian (p0) must be > 0";
    return nullptr;
}

// D = ceil(R + 0.5) - 1: the largest |dq| for which a sample of pixel p + dq can lie closer than R to the centre of p along one axis (the
// sample lies at dq + j - 0.5, j in [0, 1)).  R = D + 0.5 touches the next pixel in the one draw j = 0 only, which stays outside.
inline uint32_t pixel_filter_reach(float radius) { return (uint32_t)std::ceil((double)radius + 0.5) - 1u; }
// |offset| -> table index: one f32 division, then kx = min((uint32_t)(ax * scale), RT_FILTER_TABLE - 1) on the device.
inline float pixel_filter_scale(float radius) { return (float)RT_FILTER_TABLE / radius; }

// f(x) of the header for 0 <= x <= R, in f64, every operation in the order written here.
inline double pixel_filter_profile(const RtPixelFilter& f, double x) {
    const double R = (double)f.radius;
    switch (f.kind) {
    case RT_FILTER_TENT: return 1.0 - x / R;
    case RT_FILTER_GAUSSIAN: {
        const double s2 = 2.0 * ((double)f.p0 * (double)f.p0);
        return std::exp(-(x * x) / s2) - std::exp(-(R * R) / s2);
    }
    case RT_FILTER_MITCHELL: {
        const double B = (double)f.p0, C = (double)f.p1, t = 2.0 * x / R;
        if (t < 1.0) return (((12.0 - 9.0 * B - 6.0 * C) * t + (-18.0 + 12.0 * B + 6.0 * C)) * t * t + (6.0 - 2.0 * B)) / 6.0;
        return ((((-B - 6.0 * C) * t + (6.0 * B + 30.0 * C)) * t + (-12.0 * B - 48.0 * C)) * t + (8.0 * B + 24.0 * C)) / 6.0;
    }
    case RT_FILTER_BLACKMAN_HARRIS: {
        const double a = 3.14159265358979323846 * x / R;
        return 0.35875 + 0.48829 * std::cos(a) + 0.14128 * std::cos(2.0 * a) + 0.01168 * std::cos(3.0 * a);
    }
    default: return 1.0; // RT_FILTER_BOX
    }
}

// table[k] = (float)f(x_k) at the midpoints x_k = (k + 0.5) R / 256, `reach` = D; either output may be NULL.  NULL, or what is wrong.
inline const char* pixel_filter_table(const RtPixelFilter* f, float* table, uint32_t* reach) {
    if (const char* why = pixel_filter_invalid(f)) return why;
    if (table)
        for (uint32_t k = 0; k < RT_FILTER_TABLE; ++k) table[k] = (float)pixel_filter_profile(*f, ((double)k + 0.5) * (double)f->radius / (double)RT_FILTER_TABLE);
    if (reach) *reach = pixel_filter_reach(f->radius);
    return nullptr;
}

// Two filters are the same where their 16 bytes are (so -0 and 0 differ: a snapshot is continued bit for bit or not at all).
inline bool pixel_filter_same(const RtPixelFilter& a, const RtPixelFilter& b) {
    const unsigned char *x = reinterpret_cast<const unsigned char*>(&a), *y = reinterpret_cast<const unsigned char*>(&b);
    for (size_t k = 0; k < sizeof(RtPixelFilter); ++k)
        if (x[k] != y[k]) return false;
    return true;
}

// ---- the plane --------------------------------------------------------------------------------------------------------------------------
// (sum w r, sum w g, sum w b, sum w) per pixel: what tracking adds to an accumulation and what an RtAccumFilter carries per pixel.
constexpr size_t RT_FILTER_PIXEL_BYTES = 4 * sizeof(float);
// The accumulation's buffer: the table first, the plane of npix pixels behind it (16 B aligned).
constexpr size_t RT_FILTER_TABLE_BYTES = RT_FILTER_TABLE * sizeof(float);
inline size_t filter_buffer_bytes(uint64_t npix) { return RT_FILTER_TABLE_BYTES + (size_t)npix * RT_FILTER_PIXEL_BYTES; }

// NULL: `fs` is what rt_accum_import_filter accepts before it compares it with an accumulation.  Else: what is wrong with it.  The plane is
// not read: values are not judged.
inline const char* accum_filter_invalid(const RtAccumFilter* fs) {
    if (!fs) return "the RtAccumFilter is NULL";
    if (fs->reserved[0] != 0u || fs->reserved[1] != 0u) return "reserved must be 0";
    if (!fs->plane) return "plane must not be NULL";
    if ((uint64_t)fs->first_sample + fs->done > 0xFFFFFFFFull) return "first_sample + done must stay below 2^32, as RtParams.spp does";
    return pixel_filter_invalid(&fs->filter);
}

} // namespace rt
