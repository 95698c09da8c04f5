// rt_multiscale_plan.h — the GPU-free arithmetic of "Multi-scale denoising" (rtow_mi355x.h): the sizes of the pyramid's levels, where the
// regions of every level lie in the one buffer the host path obtains, and what makes an RtMultiscale well formed.  Like
// rt_halves_plan.h: no context, no device call, plain values in and out; tests/multiscale_plan_main.cpp runs it under AddressSanitizer +
// UBSan without a GPU.
#pragma once
#include "../../include/rtow_mi355x.h"

#include <cstddef>
#include <cstdint>

namespace rt {

// A side of the next coarser level: (side + 1) / 2 without the sum, so nothing wraps at 2^32 - 1.  A side of 1 stays 1.
inline uint32_t multiscale_half(uint32_t side) { return (side >> 1) + (side & 1u); }

// NULL: `ms` is what rt_accum_denoise_multiscale accepts (a NULL `ms` is the defaults and is not judged here).  Else: what is wrong with it.
inline const char* multiscale_invalid(const RtMultiscale* ms) {
    if (!ms) return "the RtMultiscale is NULL";
    if (ms->levels == 0u || ms->levels > RT_DENOISE_MAX_LEVELS) return "levels must be 1 .. RT_DENOISE_MAX_LEVELS";
    if (ms->guide != RT_DENOISE_GUIDE_LUMINANCE && ms->guide != RT_DENOISE_GUIDE_CHANNELS) return "guide must be RT_DENOISE_GUIDE_LUMINANCE or RT_DENOISE_GUIDE_CHANNELS";
    if (ms->reserved[0] != 0u || ms->reserved[1] != 0u) return "reserved must be 0";
    return nullptr;
}

// ---- byte sizes ---------------------------------------------------------------------------------------------------------------------------
constexpr size_t RT_MS_RGB_BYTES = 3 * sizeof(float), RT_MS_PLANE_BYTES = 2 * sizeof(float); // a colour triple; one (mean, variance) entry
constexpr size_t RT_MS_ALIGN = 256;                                                         // every region starts on a multiple of it

// Level s of the pyramid and the byte offsets of its regions, each contiguous and in image order, as launch_nlm wants them:
//   c     the colours, 12 B per pixel; with three planes the colours are the guide's means and this region is empty (c == guide)
//   guide planes x 8 B per pixel: (y, v), or (c, v) x 3
//   f     F_s, the filter's output, 12 B per pixel
//   e     the residual of level s, 12 B per pixel; empty on level 0, which has no finer level to correct
//   o     o_s, 12 B per pixel; on the coarsest level o_s IS F_s and o == f
struct MultiscaleLevel {
    uint32_t nx, rows;
    uint64_t npix;
    size_t c, guide, f, e, o;
};
struct MultiscalePlan {
    uint32_t levels, planes;
    MultiscaleLevel lv[RT_DENOISE_MAX_LEVELS];
    size_t total;
};
// levels 1 .. RT_DENOISE_MAX_LEVELS, planes 1 or 3, nx * rows 1 .. 2^28 (the callers check).  Per pixel of a level the regions take
// 12 + 8 + 12 (+ 12 + 12) B with one plane and 24 + 12 (+ 12 + 12) B with three; a level has at most (nx + 1)(rows + 1) / 4 of the pixels
// of the one below it, a quarter where both sides are even, so on a frame the levels above 0 add about a third to level 0.
inline MultiscalePlan multiscale_plan(uint32_t nx, uint32_t rows, uint32_t levels, uint32_t planes) {
    MultiscalePlan pl{};
    pl.levels = levels, pl.planes = planes;
    size_t off = 0;
    const auto take = [&off](uint64_t bytes) {
        const size_t at = off;
        off += (size_t)((bytes + (RT_MS_ALIGN - 1)) / RT_MS_ALIGN * RT_MS_ALIGN);
        return at;
    };
    for (uint32_t s = 0; s < levels; ++s) {
        MultiscaleLevel& l = pl.lv[s];
        l.nx = nx, l.rows = rows, l.npix = (uint64_t)nx * rows;
        l.c = take(planes == 1u ? l.npix * RT_MS_RGB_BYTES : 0u);
        l.guide = take(l.npix * planes * RT_MS_PLANE_BYTES);
        l.f = take(l.npix * RT_MS_RGB_BYTES);
        l.e = take(s ? l.npix * RT_MS_RGB_BYTES : 0u);
        l.o = s + 1u == levels ? l.f : take(l.npix * RT_MS_RGB_BYTES);
        nx = multiscale_half(nx), rows = multiscale_half(rows);
    }
    pl.total = off;
    return pl;
}

} // namespace rt
