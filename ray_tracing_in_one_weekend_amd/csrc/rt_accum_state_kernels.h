// rt_accum_state_kernels.h — the device side of "Accumulation state" (rtow_mi355x.h): new kernels only; no kernel of rt_kernels.h,
// rt_adaptive.h, rt_denoise.h or rt_channels.h changes, and none of these is in a variant table or a ledger family.
//
//   k_accum_export<COUNTS, CHANNELS> : the accumulation's planes (local pixel order) -> staging planes in image order
//   k_accum_import<COUNTS, CHANNELS> : staging planes in image order -> the accumulation's planes, bit for bit
//   k_accum_merge<CHANNELS>          : accumulation = accumulation + staging, one IEEE add per value (-ffp-contract=off: no FMA)
//
// One thread per pixel of the shard in image order; its local index is local_of_pixel of the accumulation's tiles_per_row and
// tile_pixels.  The image-order side of every transfer is coalesced: consecutive lanes touch consecutive 12 B, 16 B, 4 B, 1 B or 48 B
// groups.  The tile-permuted side is coalesced within the 8 lanes that share a tile row.  A 12 B group moves as three dwords in one
// access (an RGB triple is only 4 B aligned), a moment pair as one 16 B access.  COUNTS: the counts and converged planes take part
// (an adaptive accumulation); CHANNELS: the three planes of channel moments do.
#pragma once
#include "rt_kernels.h"

namespace rt {

// Three f32 that move together (4 B aligned: the compiler may use one 12 B access, never a 16 B one).
struct StateRgb {
    float r, g, b;
};

// The planes of an accumulation, in its local pixel order (rt_api.hip: accum_sum, accum_mom, accum_cnt, accum_flag, accum_chm).
struct AccumPlanes {
    float* sum;       // [npix * 3]
    double2* mom;     // [npix]
    uint32_t* cnt;    // [npix]     (COUNTS)
    uint8_t* flag;    // [npix]     (COUNTS)
    double2* chm;     // [3][npix]  (CHANNELS)
};
// The planes of a state in image order, on the device (rt_accum_state.h: accum_state_staging).
struct StagedPlanes {
    float* sum;       // [npix * 3]
    double2* mom;     // [npix]
    uint32_t* cnt;    // [npix]
    uint8_t* flag;    // [npix]
    double2* chm;     // [npix][3]: (S1_r, S2_r), (S1_g, S2_g), (S1_b, S2_b) of a pixel side by side
};

template <bool COUNTS, bool CHANNELS>
__global__ __launch_bounds__(256) void k_accum_export(AccumPlanes a, StagedPlanes s, uint32_t nx, uint32_t rows, uint32_t tiles_per_row,
                                                      uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const uint32_t npix = nx * rows;
    if (p >= npix) return;
    const size_t ap = local_of_pixel(nx, tiles_per_row, tile_pixels, p % nx, p / nx);
    reinterpret_cast<StateRgb*>(s.sum)[p] = reinterpret_cast<const StateRgb*>(a.sum)[ap];
    s.mom[p] = a.mom[ap];
    if (COUNTS) {
        s.cnt[p] = a.cnt[ap];
        s.flag[p] = a.flag[ap];
    }
    if (CHANNELS) {
        const double2 mr = a.chm[ap], mg = a.chm[(size_t)npix + ap], mb = a.chm[2 * (size_t)npix + ap];
        double2* dst = s.chm + 3 * (size_t)p;
        dst[0] = mr, dst[1] = mg, dst[2] = mb;
    }
}

template <bool COUNTS, bool CHANNELS>
__global__ __launch_bounds__(256) void k_accum_import(AccumPlanes a, StagedPlanes s, uint32_t nx, uint32_t rows, uint32_t tiles_per_row,
                                                      uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const uint32_t npix = nx * rows;
    if (p >= npix) return;
    const size_t ap = local_of_pixel(nx, tiles_per_row, tile_pixels, p % nx, p / nx);
    reinterpret_cast<StateRgb*>(a.sum)[ap] = reinterpret_cast<const StateRgb*>(s.sum)[p];
    a.mom[ap] = s.mom[p];
    if (COUNTS) {
        a.cnt[ap] = s.cnt[p];
        a.flag[ap] = s.flag[p];
    }
    if (CHANNELS) {
        const double2* src = s.chm + 3 * (size_t)p;
        const double2 mr = src[0], mg = src[1], mb = src[2];
        a.chm[ap] = mr, a.chm[(size_t)npix + ap] = mg, a.chm[2 * (size_t)npix + ap] = mb;
    }
}

__device__ __forceinline__ double2 state_add(double2 x, double2 y) { return make_double2(x.x + y.x, x.y + y.y); }

template <bool CHANNELS>
__global__ __launch_bounds__(256) void k_accum_merge(AccumPlanes a, StagedPlanes s, uint32_t nx, uint32_t rows, uint32_t tiles_per_row,
                                                     uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const uint32_t npix = nx * rows;
    if (p >= npix) return;
    const size_t ap = local_of_pixel(nx, tiles_per_row, tile_pixels, p % nx, p / nx);
    StateRgb c = reinterpret_cast<const StateRgb*>(a.sum)[ap];
    const StateRgb d = reinterpret_cast<const StateRgb*>(s.sum)[p];
    c.r = c.r + d.r, c.g = c.g + d.g, c.b = c.b + d.b;
    reinterpret_cast<StateRgb*>(a.sum)[ap] = c;
    a.mom[ap] = state_add(a.mom[ap], s.mom[p]);
    if (CHANNELS) {
        const double2* src = s.chm + 3 * (size_t)p;
        const double2 dr = src[0], dg = src[1], db = src[2];
        const double2 mr = a.chm[ap], mg = a.chm[(size_t)npix + ap], mb = a.chm[2 * (size_t)npix + ap];
        a.chm[ap] = state_add(mr, dr), a.chm[(size_t)npix + ap] = state_add(mg, dg), a.chm[2 * (size_t)npix + ap] = state_add(mb, db);
    }
}

} // namespace rt
