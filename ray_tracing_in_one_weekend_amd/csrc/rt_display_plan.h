// rt_display_plan.h — the GPU-free arithmetic of "Display transform" (rtow_mi355x.h): what makes an RtDisplay well formed
// (rt_display_check), the 8 x 8 Bayer index B, the rank of a percentile, the search of a luminance histogram for the bin that holds that
// rank, the bin's midpoint and the exposure that follows from it.  The kernels of rt_display.h call the functions below, so the device
// and the host compute with the same operations.  Like rt_halves_plan.h: no context, no device call, plain values in and out;
// tests/display_plan_main.cpp runs it under AddressSanitizer + UBSan without a GPU.
#pragma once
#include "../../include/rtow_mi355x.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RT_DISPLAY_HD __host__ __device__
#else
#define RT_DISPLAY_HD
#endif

namespace rt {

constexpr uint32_t RT_DISPLAY_BINS = 2048u;     // bits(Y) >> 20: sign 0, 8 exponent bits, the 3 leading mantissa bits — 8 bins per octave
constexpr uint32_t RT_DISPLAY_LAST_BIN = 2039u; // FLT_MAX's; +inf would be 2040 and is not lit

// NULL: `d` is what rt_set_display accepts.  Else: what is wrong with it.
inline const char* display_invalid(const RtDisplay* d) {
    if (!d) return "the RtDisplay is NULL";
    if (d->exposure_mode > RT_EXPOSURE_PERCENTILE) return "exposure_mode must be an RtExposureMode";
    if (d->curve > RT_TONE_ACES) return "curve must be an RtToneCurve";
    if (d->transfer > RT_TRANSFER_SRGB) return "transfer must be an RtTransfer";
    if (d->dither > RT_DITHER_BAYER8) return "dither must be an RtDither";
    if (!std::isfinite(d->exposure_value) || !(d->exposure_value > 0.0f)) return "exposure_value must be finite and > 0";
    if (d->exposure_mode == RT_EXPOSURE_PERCENTILE && !(d->percentile > 0.0f && d->percentile <= 1.0f)) return "percentile must lie in (0, 1]";
    if (d->curve == RT_TONE_REINHARD && !(d->white > 0.0f)) return "white must be > 0 (+inf: no white point)"; // (a NaN fails the comparison)
    if (d->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

// B(x, y), x and y in 0 .. 7: the standard 8 x 8 Bayer index, a permutation of 0 .. 63 whose first row is 0 32 8 40 2 34 10 42.
RT_DISPLAY_HD inline uint32_t display_bayer(uint32_t x, uint32_t y) {
    uint32_t b = 0u;
    for (uint32_t k = 0u; k < 3u; ++k) b |= ((((x ^ y) >> k) & 1u) << (2u * (2u - k) + 1u)) | (((y >> k) & 1u) << (2u * (2u - k)));
    return b;
}

// rank = max(1, ceil(q * n_lit)), q in (0, 1]: the product of a 24-bit and a (below 2^29) 29-bit number is exact in f64.  Never above n_lit.
RT_DISPLAY_HD inline uint64_t display_rank(float q, uint64_t n_lit) {
    const double r = ceil((double)q * (double)n_lit);
    uint64_t rank = r >= 1.0 ? (uint64_t)r : 1u;
    if (rank > n_lit && n_lit > 0u) rank = n_lit;
    return rank;
}

// The first bin whose cumulative count reaches `rank` (>= 1); RT_DISPLAY_BINS where the histogram holds fewer than `rank` pixels.
inline uint32_t display_bin_search(const uint32_t* hist, uint64_t rank) {
    uint64_t cum = 0u;
    for (uint32_t b = 0u; b < RT_DISPLAY_BINS; ++b) {
        cum += hist[b];
        if (cum >= rank) return b;
    }
    return RT_DISPLAY_BINS;
}

// The bin of a lit luminance, and L_q of a bin: the value in the middle of the bin's bit patterns.
RT_DISPLAY_HD inline uint32_t display_bin_of_bits(uint32_t y_bits) { return y_bits >> 20; }
RT_DISPLAY_HD inline uint32_t display_bin_mid_bits(uint32_t bin) { return (bin << 20) | 0x80000u; }
inline float display_bin_mid(uint32_t bin) {
    const uint32_t bits = display_bin_mid_bits(bin);
    float f;
    std::memcpy(&f, &bits, sizeof(f));
    return f;
}

// e = (float)((double)value / denominator), and 1 where that is zero or not finite (a denominator of 0, inf or NaN; a quotient that rounds to 0 or inf).
RT_DISPLAY_HD inline float display_exposure(float value, double denominator) {
    const float e = (float)((double)value / denominator);
    return (e > 0.0f && e <= 3.4028234663852886e38f) ? e : 1.0f;
}

} // namespace rt
