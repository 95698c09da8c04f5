// rt_glare_plan.h — the GPU-free arithmetic of "Glare" (rtow_mi355x.h): what makes an RtGlare well formed (rt_glare_check), the
// effective number of levels Le of a frame and the sizes of its levels, the normalised weights of the levels, and where the regions of
// the pyramid lie in the one buffer the host path obtains.  Like rt_display_plan.h: no context, no device call, plain values in and out;
// tests/glare_plan_main.cpp runs it under AddressSanitizer + UBSan without a GPU.
#pragma once
#include "../../include/rtow_mi355x.h"
#include "rt_multiscale_plan.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rt {

// NULL: `g` is what rt_set_glare accepts.  Else: what is wrong with it.  (A NaN fails every comparison below; it is named first.)
inline const char* glare_invalid(const RtGlare* g) {
    if (!g) return "the RtGlare is NULL";
    if (g->amount != g->amount || g->spread != g->spread || g->threshold != g->threshold) return "amount, spread and threshold must not be NaN";
    if (!(g->amount >= 0.0f && g->amount <= 1.0f)) return "amount must lie in [0, 1]";
    if (!(g->spread > 0.0f && g->spread <= 1.0f)) return "spread must lie in (0, 1]";
    if (!(g->threshold >= 0.0f) || !std::isfinite(g->threshold)) return "threshold must be finite and >= 0";
    if (g->levels == 0u || g->levels > RT_GLARE_MAX_LEVELS) return "levels must be 1 .. RT_GLARE_MAX_LEVELS";
    return nullptr;
}

constexpr size_t RT_GLARE_RGB_BYTES = 3 * sizeof(float);
constexpr size_t RT_GLARE_ALIGN = 256; // every region starts on a multiple of it

// Level l = 0 .. levels of the pyramid: its size, and the byte offsets of d_l and u_l (12 B per pixel, image order; level 0 stores
// neither: d_0 is recomputed from the input and U(u_1) is consumed by the combine).  w: the normalised weight of the level (level 0: 0).
struct GlareLevel {
    uint32_t nx, rows;
    uint64_t npix;
    float w;
    size_t d, u;
};
struct GlarePlan {
    uint32_t levels; // Le: min(the glare's levels, the first level whose larger side is 1); 0 for a 1 x 1 frame
    GlareLevel lv[RT_GLARE_MAX_LEVELS + 1u];
    size_t out;   // `out`, 12 B per pixel of level 0
    size_t total; // bytes
};

// Le of an nx x rows frame (both >= 1) under `levels` levels asked for.
inline uint32_t glare_levels(uint32_t nx, uint32_t rows, uint32_t levels) {
    uint32_t le = 0u;
    while (le < levels && (nx > 1u || rows > 1u)) nx = multiscale_half(nx), rows = multiscale_half(rows), ++le;
    return le;
}

// w[l - 1] = w_l / W for l = 1 .. le (le <= RT_GLARE_MAX_LEVELS): w_1 = 1, w_{l+1} = w_l * spread, W = ((w_1 + w_2) + ..) in index order,
// every operation one f32 operation.
inline void glare_weights(float spread, uint32_t le, float* w) {
    float cur = 1.0f, total = 0.0f;
    for (uint32_t l = 0; l < le; ++l) {
        w[l] = cur;
        total = l ? total + cur : cur;
        cur = cur * spread;
    }
    for (uint32_t l = 0; l < le; ++l) w[l] = w[l] / total;
}

// nx * rows 1 .. 2^28 and a glare glare_invalid accepts (the callers check).  The levels above 0 hold at most (nx + 1)(rows + 1) / 4 of
// the pixels of the one below: d and u together add about two thirds of one 12 B image to `out`.
inline GlarePlan glare_plan(uint32_t nx, uint32_t rows, const RtGlare& g) {
    GlarePlan pl{};
    pl.levels = glare_levels(nx, rows, g.levels);
    float w[RT_GLARE_MAX_LEVELS] = {};
    glare_weights(g.spread, pl.levels, w);
    size_t off = 0;
    const auto take = [&off](uint64_t bytes) {
        const size_t at = off;
        off += (size_t)((bytes + (RT_GLARE_ALIGN - 1)) / RT_GLARE_ALIGN * RT_GLARE_ALIGN);
        return at;
    };
    pl.out = take((uint64_t)nx * rows * RT_GLARE_RGB_BYTES);
    for (uint32_t l = 0; l <= pl.levels; ++l) {
        GlareLevel& v = pl.lv[l];
        v.nx = nx, v.rows = rows, v.npix = (uint64_t)nx * rows;
        v.w = l ? w[l - 1u] : 0.0f;
        v.d = take(l ? v.npix * RT_GLARE_RGB_BYTES : 0u);
        v.u = take(l ? v.npix * RT_GLARE_RGB_BYTES : 0u);
        nx = multiscale_half(nx), rows = multiscale_half(rows);
    }
    pl.total = off;
    return pl;
}

} // namespace rt
