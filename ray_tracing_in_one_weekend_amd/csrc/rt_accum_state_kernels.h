// rt_accum_state_kernels.h — the device side of "Accumulation state" (rtow_mi355x.h) and of every other snapshot of an accumulation; no
// kernel of rt_kernels.h, rt_adaptive.h, rt_denoise.h or rt_channels.h changes, and none of these is in a variant table or a ledger family.
//
//   k_planes_move<EXPORT>   : the planes of a PlaneTable (rt_accum_planes.h) between the accumulation's local pixel order and the staging
//                             buffer in image order, bit for bit — EXPORT: local -> staging, else staging -> local.  A state, the halves
//                             and the buckets all move through it.
//   k_accum_merge<CHANNELS> : accumulation = accumulation + staging, one IEEE add per value (-ffp-contract=off: no FMA)
//
// One thread per pixel of the shard in image order; its local index is local_of_pixel of the accumulation's tiles_per_row and
// tile_pixels.  The image-order side of every transfer is coalesced: consecutive lanes touch consecutive 12 B, 16 B, 4 B, 1 B or 48 B
// groups.  The tile-permuted side is coalesced within the 8 lanes that share a tile row.  A 12 B group moves as three dwords in one
// access (an RGB triple is only 4 B aligned), a moment pair as one 16 B access.
#pragma once
#include "rt_accum_planes.h"
#include "rt_kernels.h"

namespace rt {

// Three f32 that move together (4 B aligned: the compiler may use one 12 B access, never a 16 B one).
struct StateRgb {
    float r, g, b;
};

template <bool EXPORT, class T>
__device__ __forceinline__ void plane_move(char* local, char* image, size_t lp, size_t ip) {
    T *l = reinterpret_cast<T*>(local) + lp, *i = reinterpret_cast<T*>(image) + ip;
    if (EXPORT) *i = *l;
    else *l = *i;
}
// The channel moments: three 16 B parts, part k at local[k * npix] and at image[k], all loaded before the first is stored (in named
// registers: hipcc puts an array indexed by the part into scratch and LDS).
template <bool EXPORT>
__device__ __forceinline__ void plane_move_three(uint4* local, uint4* image, size_t npix) {
    const uint4 a = EXPORT ? local[0] : image[0], b = EXPORT ? local[npix] : image[1], c = EXPORT ? local[2 * npix] : image[2];
    if (EXPORT) image[0] = a, image[1] = b, image[2] = c;
    else local[0] = a, local[npix] = b, local[2 * npix] = c;
}

// The table is a kernel argument by value: its rows, and so the element size the switch goes by, are the same for every lane.
template <bool EXPORT>
__global__ __launch_bounds__(256) void k_planes_move(PlaneTable t, char* stage, uint32_t nx, uint32_t rows, uint32_t tiles_per_row, uint32_t tile_pixels) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const uint32_t npix = nx * rows;
    if (p >= npix) return;
    const size_t ap = local_of_pixel(nx, tiles_per_row, tile_pixels, p % nx, p / nx);
    for (uint32_t k = 0; k < t.n; ++k) {
        const Plane pl = t.row[k];
        char *local = static_cast<char*>(pl.local), *image = stage + pl.stage;
        if (pl.elem_bytes == 16u && pl.parts == 3u) {
            plane_move_three<EXPORT>(reinterpret_cast<uint4*>(local) + ap, reinterpret_cast<uint4*>(image) + 3 * (size_t)p, npix);
            continue;
        }
        for (uint32_t part = 0; part < pl.parts; ++part) {
            const size_t lp = (size_t)part * npix + ap, ip = (size_t)p * pl.parts + part;
            switch (pl.elem_bytes) {
            case 1u: plane_move<EXPORT, uint8_t>(local, image, lp, ip); break;
            case 4u: plane_move<EXPORT, uint32_t>(local, image, lp, ip); break;
            case 12u: plane_move<EXPORT, StateRgb>(local, image, lp, ip); break;
            default: plane_move<EXPORT, uint4>(local, image, lp, ip); break;
            }
        }
    }
}

// The planes of an accumulation, in its local pixel order (rt_api.hip: accum_sum, accum_mom, accum_cnt, accum_flag, accum_chm).
struct AccumPlanes {
    float* sum;       // [npix * 3]
    double2* mom;     // [npix]
    uint32_t* cnt;    // [npix]     (an adaptive accumulation)
    uint8_t* flag;    // [npix]     (an adaptive accumulation)
    double2* chm;     // [3][npix]  (one that tracks channels)
};
// What k_accum_merge reads of a state in image order: the rows of its table in the staging buffer.
struct StagedPlanes {
    float* sum;       // [npix * 3]
    double2* mom;     // [npix]
    uint32_t* cnt;    // (no merge of counts)
    uint8_t* flag;
    double2* chm;     // [npix][3]: (S1_r, S2_r), (S1_g, S2_g), (S1_b, S2_b) of a pixel side by side
};

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
