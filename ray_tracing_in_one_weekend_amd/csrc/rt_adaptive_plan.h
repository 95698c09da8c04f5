// rt_adaptive_plan.h — the GPU-free arithmetic of adaptive sampling (rtow_mi355x.h "Adaptive sampling"): the ranges of an RtAdaptive, the
// f64 figures of one pixel and the stopping criterion.  k_adaptive_decide (rt_adaptive.h) calls the very functions below, so the device and
// the host decide with the same operations in the same order (-ffp-contract=off on both sides: no FMA).  Like rt_frame_plan.h: no context,
// no device call, plain values in and out; tests/adaptive_plan_main.cpp runs it under AddressSanitizer + UBSan without a GPU.
#pragma once
#include "../../include/rtow_mi355x.h"

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RT_ADAPTIVE_HD __host__ __device__
#else
#define RT_ADAPTIVE_HD
#endif

namespace rt {

// NULL: `ad` and `n_samples` are what rt_accum_add_adaptive accepts.  Else: what is wrong with them.
inline const char* adaptive_invalid(const RtAdaptive* ad, uint32_t n_samples) {
    if (!ad) return "the RtAdaptive is NULL";
    if (n_samples == 0u) return "n_samples must be > 0";
    if (!std::isfinite(ad->tolerance) || !(ad->tolerance >= 0.0)) return "tolerance must be finite and >= 0";
    if (!std::isfinite(ad->luminance_floor) || !(ad->luminance_floor > 0.0)) return "luminance_floor must be finite and > 0";
    if (ad->min_samples < 2u) return "min_samples must be >= 2 (one sample has no variance estimate)";
    if (ad->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

// Mean luminance and variance of the mean of one pixel after n samples ("Moments"; pixel_noise of rt_kernels.h, operation for operation).
RT_ADAPTIVE_HD inline void adaptive_pixel_figures(double s1, double s2, uint32_t n, double& ybar, double& v) {
    const double dn = (double)n;
    ybar = n ? s1 / dn : 0.0;
    v = 0.0;
    if (n >= 2u) {
        const double q = (s2 - s1 * s1 / dn) / (dn - 1.0);
        v = (q < 0.0 ? 0.0 : q) / dn; // (a NaN stays one)
    }
}

// The criterion: thr = tolerance * max(Ybar, luminance_floor), max(a, b) = a > b ? a : b; converged iff n >= min_samples && V <= thr * thr.
// A pixel that holds a non-finite sample has a NaN V from two samples on (S2 - S1 S1 / n is inf - inf or NaN), and V <= x is false for a NaN:
// such a pixel never converges, whatever the maximum picked.
RT_ADAPTIVE_HD inline bool adaptive_converged(double ybar, double v, uint32_t n, double tolerance, double luminance_floor, uint32_t min_samples) {
    const double m = ybar > luminance_floor ? ybar : luminance_floor;
    const double thr = tolerance * m;
    return n >= min_samples && v <= thr * thr;
}
inline bool adaptive_converged_moments(double s1, double s2, uint32_t n, const RtAdaptive& ad) {
    double ybar, v;
    adaptive_pixel_figures(s1, s2, n, ybar, v);
    return adaptive_converged(ybar, v, n, ad.tolerance, ad.luminance_floor, ad.min_samples);
}

} // namespace rt
