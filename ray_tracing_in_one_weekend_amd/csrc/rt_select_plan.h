// rt_select_plan.h — the GPU-free arithmetic of "Selected strength" (rtow_mi355x.h): what makes an RtSelect well formed (rt_select_check),
// the defaults, the window and clamp arithmetic the kernels of rt_select.h share with the host, and where the planes of a run lie in its
// one buffer.  Like rt_halves_plan.h: no context, no device call, plain values in and out; tests/select_plan_main.cpp runs it under
// AddressSanitizer + UBSan without a GPU.
#pragma once
#include "../../include/rtow_mi355x.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RT_SELECT_HD __host__ __device__
#else
#define RT_SELECT_HD
#endif

namespace rt {

// `sel` NULL of rt_accum_denoise_select
// (of the candidate sets and windows measured on rendered frames the one that is more than 5 % better than every other on both: DESIGN.md
// "Selected strength")
inline RtSelect select_defaults() { return RtSelect{3u, {0.7f, 1.0f, 1.4f, 0.0f}, 5u, 1u, 0u, 1u, 0u}; }

// NULL: `sel` is what rt_accum_denoise_select accepts (a NULL `sel` stands for the defaults).  Else: what is wrong with it.
inline const char* select_invalid(const RtSelect* sel) {
    if (!sel) return nullptr;
    if (sel->n_strengths < 2u || sel->n_strengths > RT_SELECT_MAX) return "n_strengths must be 2 .. RT_SELECT_MAX";
    for (uint32_t j = 0; j < sel->n_strengths; ++j) {
        if (!std::isfinite(sel->strength[j]) || !(sel->strength[j] > 0.0f)) return "every strength must be finite and > 0";
        if (j && !(sel->strength[j - 1u] < sel->strength[j])) return "the strengths must be strictly increasing";
    }
    if (sel->radius == 0u || sel->radius > RT_DENOISE_MAX_RADIUS) return "radius must be 1 .. RT_DENOISE_MAX_RADIUS";
    if (sel->patch > RT_DENOISE_MAX_PATCH) return "patch must be 0 .. RT_DENOISE_MAX_PATCH";
    if (sel->error_radius > RT_SELECT_MAX_WINDOW) return "error_radius must be 0 .. RT_SELECT_MAX_WINDOW";
    if (sel->blend_radius > RT_SELECT_MAX_WINDOW) return "blend_radius must be 0 .. RT_SELECT_MAX_WINDOW";
    if (sel->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

// ---- windows: a workgroup of 16 x 16 pixels and its halo ------------------------------------------------------------------------------------
constexpr uint32_t RT_SEL_TILE = 16u;
constexpr uint32_t RT_SEL_SIDE_MAX = RT_SEL_TILE + 2u * RT_SELECT_MAX_WINDOW; // 24: the side of a tile with the largest halo
// The side of the tile with a halo of `halo` pixels, and the number of pixels of a (2 halo + 1)^2 window.
RT_SELECT_HD inline uint32_t select_side(uint32_t halo) { return RT_SEL_TILE + 2u * halo; }
RT_SELECT_HD inline uint32_t select_window(uint32_t halo) { return (2u * halo + 1u) * (2u * halo + 1u); }
// The image coordinate behind tile entry l of the workgroup `block` along an axis of n pixels: clamped per axis, as the header clamps p + o.
RT_SELECT_HD inline uint32_t select_clamp(uint32_t block, uint32_t l, uint32_t halo, uint32_t n) {
    const int64_t v = (int64_t)block * RT_SEL_TILE + l - halo;
    return v < 0 ? 0u : (v >= (int64_t)n ? n - 1u : (uint32_t)v);
}

// ---- frame figures: what a workgroup of 256 pixels hands to the final kernel -------------------------------------------------------------------
struct SelectPartial {
    double e[RT_SELECT_MAX + 1u];   // sum E_j over its usable pixels, j < K; [RT_SELECT_MAX]: sum E_{s(p)}(p)
    uint32_t n[RT_SELECT_MAX + 1u]; // pixels with s(p) = j; [RT_SELECT_MAX]: usable pixels
    uint32_t pad;
};
static_assert(sizeof(SelectPartial) == 64u, "one partial is 64 B");

// ---- the buffer of a run -----------------------------------------------------------------------------------------------------------------------
// Byte offsets of the regions for npix pixels and K candidates, each aligned to 16 B: the partials and the figures; the inputs (c_h 12 B,
// (y, v)_h 8 B, the counts of the debug hook 4 B); K planes of f_{j,0} and of f_{j,1} (12 B each); K planes of out_j (12 B) and of
// E_j (4 B); est (4 B), out (12 B), the index (1 B).
struct SelectLayout {
    size_t partials, info, c[2], yv[2], cnt, f[2][RT_SELECT_MAX], out_j[RT_SELECT_MAX], e_j[RT_SELECT_MAX], est, out, index, total;
    uint32_t n_partials;
};
inline SelectLayout select_layout(uint64_t npix, uint32_t K) {
    SelectLayout l{};
    size_t off = 0;
    const auto take = [&](size_t bytes) {
        const size_t at = off;
        off += (bytes + 15u) & ~(size_t)15u;
        return at;
    };
    l.n_partials = (uint32_t)((npix + 255u) / 256u);
    l.partials = take((size_t)l.n_partials * sizeof(SelectPartial));
    l.info = take(sizeof(RtSelectInfo));
    for (int h = 0; h < 2; ++h) l.c[h] = take((size_t)npix * 12u);
    for (int h = 0; h < 2; ++h) l.yv[h] = take((size_t)npix * 8u);
    l.cnt = take((size_t)npix * 4u);
    for (int h = 0; h < 2; ++h)
        for (uint32_t j = 0; j < K; ++j) l.f[h][j] = take((size_t)npix * 12u);
    for (uint32_t j = 0; j < K; ++j) l.out_j[j] = take((size_t)npix * 12u);
    for (uint32_t j = 0; j < K; ++j) l.e_j[j] = take((size_t)npix * 4u);
    l.est = take((size_t)npix * 4u);
    l.out = take((size_t)npix * 12u);
    l.index = take((size_t)npix);
    l.total = off;
    return l;
}

} // namespace rt
