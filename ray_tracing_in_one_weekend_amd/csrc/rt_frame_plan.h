// rt_frame_plan.h — host-side arithmetic of a frame: which rows a shard owns, how large a slice may be, where its work buffers lie,
// in which order the pixels are enumerated, and the GenParams the kernels invert a slot with.
//
// The kernels trust all of it without checking: a slot's inverse mapping (path_key_of_slot, gen_primary) is right only while quotients
// stay below 2^21 and npix * S <= 0xFFFFFF00, slice_fit only while a ray costs at least 100 B, and the work buffers stay apart only if
// work_layout says so.  Like rt_scene_prep.h this is host arithmetic only: no context, no device call, plain values in and out, so
// rt_api.hip decides a frame here before it enqueues anything, and tests/frame_plan_main.hip holds the same code against brute force
// under AddressSanitizer + UBSan without a GPU.
#pragma once
#include "../../include/rtow_mi355x.h"
#include "rt_kernels.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace rt {

// ---- the rows of a shard ---------------------------------------------------------------------------------------
// (rt_shard_rows of rtow_mi355x.h)
inline uint32_t shard_rows(uint32_t ny, uint32_t shard_band, uint32_t shard_count, uint32_t shard_id) {
    if (shard_count <= 1) return ny;
    if (shard_band == 0) shard_band = 1;
    if (shard_id >= shard_count) return 0;
    // rows j with (j / band) % count == id: `band` rows out of every cycle of band * count, plus what the last partial cycle holds
    const uint64_t cycle = (uint64_t)shard_band * shard_count;
    const uint64_t rem = ny % cycle, lo = (uint64_t)shard_id * shard_band;
    return (uint32_t)((ny / cycle) * shard_band + (rem > lo ? std::min<uint64_t>(rem - lo, shard_band) : 0u));
}
// The shard of a frame with the defaults of RtParams applied (shard_band 0: 1, shard_count 0: 1), its local rows and pixels.
struct ShardGeom {
    uint32_t band, count, id, rows;
    uint64_t npix64;
};
inline ShardGeom shard_geom(const RtParams& p) {
    ShardGeom g;
    g.band = p.shard_band ? p.shard_band : 1u;
    g.count = p.shard_count <= 1 ? 1u : p.shard_count;
    g.id = p.shard_id;
    g.rows = shard_rows(p.ny, g.band, p.shard_count, p.shard_id);
    g.npix64 = (uint64_t)g.rows * p.nx;
    return g;
}

// ---- work buffers of a slice -------------------------------------------------------------------------------------
// Where the work buffers of a slice lie in the pool: two ray queues of n_queue rays (a / b records interleaved when RT_QSTRIDE is
// 2, a separate b array in the RT_QSTRIDE 1 build; the c array), n_queue hit records, n_paths radiance slots.
struct WorkLayout {
    size_t q_ab[2], q_b[2], q_c[2], qhit, rad, total;
};
inline WorkLayout work_layout(size_t n_queue, size_t n_paths) {
    WorkLayout w{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 255u) & ~(size_t)255u;
        return o;
    };
    for (int k = 0; k < 2; ++k) {
        w.q_ab[k] = take(RT_QSTRIDE * n_queue * sizeof(float4));
        w.q_b[k] = RT_QSTRIDE == 1u ? take(n_queue * sizeof(float4)) : w.q_ab[k] + sizeof(float4);
        w.q_c[k] = take(n_queue * sizeof(float2));
    }
    w.qhit = take(n_queue * sizeof(float2));
    w.rad = take(n_paths * RT_RAD_FLOATS * sizeof(float));
    w.total = off;
    return w;
}

// Capacity of one of the nq queue shards of a slice of n_max rays: the rays are dealt to the shards in chunks of 256, round robin.
inline uint32_t shard_cap(uint32_t nq, uint32_t n_max) {
    const uint32_t nchunks = (n_max + 255u) / 256u;
    return ((nchunks + nq - 1) / nq) * 256u;
}

// ---- slice sizing (rt_prepare, rt_accum_begin and trace_samples) ------------------------------------------------
// A ray of a slice costs 100 B of work buffers (two 40 B queues, 8 B hit record, 12 B radiance slot).  Few, large slices amortise
// the short-queue tail of the bounce loop (depths > ~12 hold a few thousand rays: config 2 measured 99 / 88 / 82 / 79.5 ms per
// frame with 8 / 4 / 2 / 1 slices), so the library's own choice is up to 1 280 Mi rays (134 GB of the 288 GB HBM) and never more
// than half of what the device has free.
#ifndef RT_MAX_SLICE_MI_RAYS
#define RT_MAX_SLICE_MI_RAYS 1280 // Mi rays of the largest slice the library chooses by itself (134 GB of work buffers).  640 until round 6:
                                  // config 3 (4K, 1024 spp) in 7 slices instead of 13 is 1.6 % faster, config 5 1 % (the tail of a slice costs 3.7 ms)
#endif
inline size_t slice_bytes(uint32_t nq, uint32_t npix, uint32_t sc) {
    const uint32_t n_max = npix * sc;
    return work_layout((size_t)nq * shard_cap(nq, n_max), n_max).total;
}
// the most samples per pixel (<= sc_max) whose slice fits `bytes`; 0 when not even one does
inline uint32_t slice_fit(uint32_t nq, uint32_t npix, size_t bytes, uint32_t sc_max) {
    uint32_t sc = (uint32_t)std::min<uint64_t>(sc_max, bytes / (100ull * npix) + 1u);
    while (sc > 0u && slice_bytes(nq, npix, sc) > bytes) --sc;
    return sc;
}
struct SlicePlan {
    uint32_t S_cap;    // most samples per pixel a slice may hold
    bool by_library;   // RtParams.spp_slice == 0: the library chose, and may start a frame with smaller slices while the pool grows
    size_t want_bytes; // pool size that holds such a slice
};
// The slices of a frame of npix64 pixels whose work buffers start at `work_base` of the pool.  free_bytes: what the device has free
// beside the mapped_bytes the pool holds already (read only for a size the library chooses; SIZE_MAX: unknown, no bound from it).
// false: not even one sample per pixel stays within the slot arithmetic.
inline bool plan_slice_size(const RtParams& prm, uint64_t npix64, uint32_t nq, size_t free_bytes, size_t mapped_bytes, size_t work_base, SlicePlan& pl) {
    const uint32_t spp = prm.spp;
    uint32_t S = prm.spp_slice;
    pl.by_library = S == 0u;
    if (pl.by_library) S = (uint32_t)std::max<uint64_t>(1, ((uint64_t)RT_MAX_SLICE_MI_RAYS << 20) / npix64);
    S = std::min(std::min(S, spp), 1u << 20); // udiv_inv (slot -> sample, pixel) wants quotients below 2^21
    if ((uint64_t)S * npix64 > 0xFFFFFF00ull) S = (uint32_t)(0xFFFFFF00ull / npix64);
    if (S == 0) return false;
    const uint32_t npix = (uint32_t)npix64;
    if (pl.by_library && free_bytes != SIZE_MAX) {
        const size_t half = (free_bytes + mapped_bytes) / 2u, base = work_base;
        if (base + slice_bytes(nq, npix, S) > half) S = std::max(1u, slice_fit(nq, npix, half > base ? half - base : 0u, S));
    }
    pl.S_cap = S;
    pl.want_bytes = work_base + slice_bytes(nq, npix, S);
    return true;
}

// ---- pixel order and GenParams ---------------------------------------------------------------------------------
// Local pixel order of a shard's frame (rt_kernels.h GenParams): 8 x 8 pixel tiles per wave of depth 0 when the frame allows it.  A strip
// of 64 x 1 pixels crosses more silhouettes than a block of 8 x 8, and at depth 0 a wave runs the union of what its lanes hit.  Frames are
// bit-identical (keys and the resolve order are functions of (pixel, sample)).  sphere_scene: depth-0 shading 7.17 -> 6.67 ms
// per 128 spp, frame 58.6 -> 57.4 ms; pbr_sweep_scene -1.5 %; cornell_box +-0; final_scene +1.7 % (its deeper bounces,
// 42.0 -> 43.6 ms of k_intersect), so general scenes keep the rows (profiles/round3/ab_tiles.txt).
struct PixelOrder {
    uint32_t tiles_per_row, tile_pixels;
};
inline PixelOrder pixel_order(uint32_t po, bool general_scene, uint32_t nx, uint32_t rows) { // po = RT_OPT_PIXEL_ORDER: 1 = rows, 2 = tiles wherever the frame allows
    const bool want_tiles = po ? po == 2u : !general_scene;
    PixelOrder o;
    o.tiles_per_row = (nx % 8u == 0u && rows >= 8u && want_tiles) ? nx / 8u : 0u;
    o.tile_pixels = o.tiles_per_row * 64u * (rows / 8u); // the last rows % 8 rows stay row-major
    return o;
}

// udiv_inv (rt_kernels.h): the reciprocal that keeps the float quotient at or below the true one
inline float udiv_reciprocal(uint32_t d) { return (float)((1.0 / (double)d) * (1.0 - 1.0 / 4194304.0)); }

// The GenParams of a frame.  What changes from slice to slice (cap, s0, n_rays) and the candidate lists are the caller's.
inline GenParams frame_gen_params(const RtCamera& cam, const RtParams& prm, const ShardGeom& sh, uint32_t nq, const PixelOrder& po) {
    GenParams gp{};
    for (int k = 0; k < 3; ++k) {
        gp.cam_origin[k] = cam.origin[k];
        gp.cam_horizontal[k] = cam.horizontal[k];
        gp.cam_vertical[k] = cam.vertical[k];
        gp.cam_llc[k] = cam.lower_left_corner[k];
    }
    const uint32_t npix = (uint32_t)sh.npix64;
    gp.nx = prm.nx, gp.ny = prm.ny, gp.npix = npix;
    gp.shard_band = sh.band, gp.shard_count = sh.count, gp.shard_id = sh.id;
    gp.nq = nq, gp.cap = 0u; // (cap: per slice)
    gp.seed_lo = (uint32_t)prm.seed, gp.seed_hi = (uint32_t)(prm.seed >> 32);
    gp.lists = nullptr;
    gp.n_overflow = nullptr;
    gp.inv_npix = udiv_reciprocal(npix), gp.inv_nx = udiv_reciprocal(prm.nx), gp.inv_band = udiv_reciprocal(sh.band);
    gp.tiles_per_row = po.tiles_per_row, gp.tile_pixels = po.tile_pixels;
    gp.inv_tpr = po.tiles_per_row ? udiv_reciprocal(po.tiles_per_row) : 0.0f;
    return gp;
}

} // namespace rt
