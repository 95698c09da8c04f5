// rt_accum_state.h — the GPU-free part of "Accumulation state" (rtow_mi355x.h): the identity of a frame (rt_accum_frame_id), what makes an
// RtAccumState well formed (rt_accum_state_check) and the byte sizes of its planes.  Like rt_adaptive_plan.h and rt_frame_plan.h: no
// context, no device call, plain values in and out; rt_api.hip calls the functions below before it enqueues anything, and
// tests/accum_state_main.cpp runs them under AddressSanitizer + UBSan without a GPU.
#pragma once
#include "../../include/rtow_mi355x.h"

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace rt {

// ---- the identity of a frame ------------------------------------------------------------------------------------------------------------
// FNV-1a 64 over little-endian bytes, least significant byte of a value first whatever the host's byte order.
struct Fnv1a64 {
    uint64_t h = 0xcbf29ce484222325ull;
    void byte(uint8_t b) { h = (h ^ b) * 0x100000001b3ull; }
    void u32(uint32_t v) {
        for (int k = 0; k < 4; ++k) byte((uint8_t)(v >> (8 * k)));
    }
    void u64(uint64_t v) {
        for (int k = 0; k < 8; ++k) byte((uint8_t)(v >> (8 * k)));
    }
    void f32(float f) {
        uint32_t v;
        std::memcpy(&v, &f, sizeof(v));
        u32(v);
    }
};

// Everything a sample's value hangs on that RtCamera and RtParams carry: the 12 camera floats as bit patterns in struct order, nx, ny,
// max_depth, the seed, the shard (an unsharded frame is (0, 1, 0) however it was written) and the Russian-roulette bit.  Not spp, spp_slice,
// RT_FLAG_BRUTE_FORCE or the diagnostic bits: no result depends on them.
inline uint64_t accum_frame_id(const RtCamera& cam, const RtParams& p) {
    Fnv1a64 f;
    for (int k = 0; k < 3; ++k) f.f32(cam.origin[k]);
    for (int k = 0; k < 3; ++k) f.f32(cam.horizontal[k]);
    for (int k = 0; k < 3; ++k) f.f32(cam.vertical[k]);
    for (int k = 0; k < 3; ++k) f.f32(cam.lower_left_corner[k]);
    f.u32(p.nx), f.u32(p.ny), f.u32((uint32_t)p.max_depth);
    f.u64(p.seed);
    const bool sharded = p.shard_count > 1u;
    f.u32(sharded ? p.shard_band : 0u), f.u32(sharded ? p.shard_count : 1u), f.u32(sharded ? p.shard_id : 0u);
    f.u32(p.flags & RT_FLAG_RUSSIAN_ROULETTE);
    return f.h;
}

// ---- a well-formed state ----------------------------------------------------------------------------------------------------------------
inline uint64_t accum_state_pixels(const RtAccumState& st) { return (uint64_t)st.nx * st.rows; }

// NULL: `st` is what rt_accum_import and rt_accum_merge accept before they compare it with an accumulation.  Else: what is wrong with it.
// The planes are read only as far as the scalar fields say they reach.
inline const char* accum_state_invalid(const RtAccumState* st) {
    if (!st) return "the RtAccumState is NULL";
    if (st->reserved != 0u) return "reserved must be 0";
    if (st->planes & ~(RT_ACCUM_STATE_COUNTS | RT_ACCUM_STATE_CHANNELS)) return "planes holds a bit that is no RT_ACCUM_STATE_*";
    if (!st->sum || !st->moments) return "sum and moments must not be NULL";
    const bool counts = (st->planes & RT_ACCUM_STATE_COUNTS) != 0u, channels = (st->planes & RT_ACCUM_STATE_CHANNELS) != 0u;
    if (counts != (st->counts != nullptr) || counts != (st->converged != nullptr))
        return "counts and converged must be non-NULL exactly when planes holds RT_ACCUM_STATE_COUNTS";
    if (channels != (st->channel_moments != nullptr)) return "channel_moments must be non-NULL exactly when planes holds RT_ACCUM_STATE_CHANNELS";
    if ((uint64_t)st->first_sample + st->done > 0xFFFFFFFFull) return "first_sample + done must stay below 2^32, as RtParams.spp does";
    if (counts) {
        const uint64_t npix = accum_state_pixels(*st);
        for (uint64_t p = 0; p < npix; ++p) {
            if (st->converged[p] > 1u) return "converged holds a value that is neither 0 nor 1";
            if (st->counts[p] > st->done) return "a pixel counts more samples than were issued (counts[p] > done)";
            if (st->converged[p] == 0u && st->counts[p] != st->done) return "an active pixel does not hold every issued sample (counts[p] != done)";
        }
    }
    return nullptr;
}

// ---- byte sizes -------------------------------------------------------------------------------------------------------------------------
constexpr size_t RT_STATE_SUM_BYTES = 3 * sizeof(float), RT_STATE_MOMENT_BYTES = 2 * sizeof(double), RT_STATE_COUNT_BYTES = sizeof(uint32_t),
                 RT_STATE_FLAG_BYTES = sizeof(uint8_t), RT_STATE_CHANNEL_BYTES = 6 * sizeof(double);
// Bytes per pixel of a state with the planes `planes`: 28, + 5 with counts, + 48 with channel moments.
inline size_t accum_state_pixel_bytes(uint32_t planes) {
    return RT_STATE_SUM_BYTES + RT_STATE_MOMENT_BYTES + ((planes & RT_ACCUM_STATE_COUNTS) ? RT_STATE_COUNT_BYTES + RT_STATE_FLAG_BYTES : 0u) +
           ((planes & RT_ACCUM_STATE_CHANNELS) ? RT_STATE_CHANNEL_BYTES : 0u);
}
inline uint64_t accum_state_bytes(uint64_t npix, uint32_t planes) { return npix * accum_state_pixel_bytes(planes); }

} // namespace rt
