// rt_multi_accum_plan.h — the GPU-free part of "Progressive accumulation across devices" (rtow_mi355x.h, rt_multi_accum_*): which image row
// a shard's local row is, where the tables of a shard's planes lie in its send buffer and in its slot of the first device's gather buffer,
// and the split of a whole-frame snapshot into the snapshots of the n shards (rt_multi_accum_import).  Like rt_accum_planes.h: no context,
// no device call, plain values in and out; tests/multi_accum_plan_main.cpp runs it under AddressSanitizer + UBSan without a GPU.
#pragma once
#include "rt_accum_planes.h"

#include <algorithm>
#include <memory>

namespace rt {

// ---- the row map ------------------------------------------------------------------------------------------------------------------------
// rt_multi_*: rows per band, RtParams.shard_band with 0 = 8
inline uint32_t multi_band(uint32_t shard_band) { return shard_band ? shard_band : 8u; }
// Local row lj of shard r of n -> image row (rt_shard_row_to_image_row; k_planes_join and k_bands_to_image compute the same)
inline uint32_t multi_image_row(uint32_t lj, uint32_t band, uint32_t n, uint32_t r) { return n <= 1u ? lj : ((lj / band) * n + r) * band + lj % band; }
// The local rows of shard r of n: rt_shard_rows restated (rt_frame_plan.h needs the device headers; this file does not), the rows lj with
// multi_image_row(lj) < ny — `band` rows of every whole cycle of band * n rows, plus what the last, partial cycle holds of band r
inline uint32_t multi_shard_rows(uint32_t ny, uint32_t band, uint32_t n, uint32_t r) {
    if (n <= 1u) return ny;
    if (r >= n) return 0u;
    const uint64_t cycle = (uint64_t)band * n, rem = ny % cycle, lo = (uint64_t)r * band;
    return (uint32_t)((ny / cycle) * band + (rem > lo ? std::min<uint64_t>(rem - lo, band) : 0u));
}
// The rows of the largest shard: every slot of the gather buffer is laid out for this many
inline uint32_t multi_rows_pad(uint32_t ny, uint32_t band, uint32_t n) {
    uint32_t rows_pad = 0;
    for (uint32_t r = 0; r < n; ++r) rows_pad = std::max(rows_pad, multi_shard_rows(ny, band, n, r));
    return rows_pad;
}

// ---- the tables of a shard in one buffer ------------------------------------------------------------------------------------------------
// What an accumulation holds beside the 28 B of sum and moments
struct MultiTracked {
    bool counts, channels, halves;
    uint32_t buckets; // M, 0: none
};
constexpr uint32_t RT_MULTI_TABLES = 3u; // state, halves, buckets
// The three tables over the planes of an accumulation whose planes hold npix_local pixels each (local pointers as rt_api.hip holds them;
// NULL where the caller only wants sizes).  A table that is not tracked has no rows.
struct MultiTables {
    PlaneTable t[RT_MULTI_TABLES];
    size_t base[RT_MULTI_TABLES]; // where a table's planes begin in the buffer: its rows' `stage` counts from here; 16 B aligned
    size_t bytes;                 // of the buffer
};
inline MultiTables multi_tables(const MultiTracked& tr, void* sum, void* mom, void* cnt, void* flag, void* chm, void* halves, void* buckets, uint64_t npix_local) {
    MultiTables mt{};
    mt.t[0] = state_planes(RtAccumState{}, tr.counts, tr.channels, sum, mom, cnt, flag, chm);
    if (tr.halves) mt.t[1] = halves_planes(RtAccumHalves{}, halves, npix_local);
    if (tr.buckets) mt.t[2] = buckets_planes(RtAccumBuckets{}, tr.buckets, buckets, npix_local);
    return mt;
}
// Places the tables one behind the other for npix pixels (planes_place each), every base rounded up to 16 B; returns the buffer's size.
inline size_t multi_place(MultiTables& mt, uint64_t npix) {
    size_t off = 0;
    for (uint32_t k = 0; k < RT_MULTI_TABLES; ++k) {
        off = (off + 15u) & ~(size_t)15u;
        mt.base[k] = off;
        off += planes_place(mt.t[k], npix);
    }
    return mt.bytes = off;
}
// The bytes a shard of npix pixels sends, and the stride of the slots: the layout at rows_pad rows, a multiple of 16 B.  A shard's own
// layout is never longer (every table's size grows with npix), so slot r holds shard r's buffer as it is.
inline size_t multi_shard_bytes(const MultiTracked& tr, uint64_t npix) {
    MultiTables mt = multi_tables(tr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, npix);
    return multi_place(mt, npix);
}
inline size_t multi_slot_stride(const MultiTracked& tr, uint32_t nx, uint32_t rows_pad) {
    return (multi_shard_bytes(tr, (uint64_t)nx * rows_pad) + 15u) & ~(size_t)15u;
}

// ---- a whole-frame snapshot split into the shards' ---------------------------------------------------------------------------------------
// An array of exactly n elements (n = 0: a pointer that is not NULL and may not be read)
template <class T>
struct HostPlane {
    std::unique_ptr<T[]> p;
    void take(const T* whole, uint32_t per_pixel, uint32_t nx, uint32_t rows, uint32_t band, uint32_t n, uint32_t r) {
        const size_t row = (size_t)nx * per_pixel;
        p.reset(new T[row * rows]);
        for (uint32_t lj = 0; lj < rows; ++lj) std::memcpy(p.get() + lj * row, whole + multi_image_row(lj, band, n, r) * row, row * sizeof(T));
    }
};
// The snapshots of shard r: the scalar fields of the whole frame's with rows and frame_id the shard's, and the shard's rows of every plane
struct ShardSnapshot {
    RtAccumState st{};
    RtAccumHalves hs{};
    RtAccumBuckets bs{};
    HostPlane<float> sum, hsum[2], bsum[RT_BUCKETS_MAX];
    HostPlane<double> moments, channel_moments, hmoments[2];
    HostPlane<uint32_t> counts;
    HostPlane<uint8_t> converged;
};
// The params of shard r of n of the frame of `prm` (what device r's accumulation is begun with)
inline RtParams multi_shard_params(const RtParams& prm, uint32_t n, uint32_t r) {
    RtParams p = prm;
    p.shard_band = multi_band(prm.shard_band), p.shard_count = n, p.shard_id = r;
    return p;
}
// `whole` (well formed: accum_state_invalid) is a state of the ny rows of the frame of (cam, prm); hs / bs NULL or well formed over the
// same rows.  out.hs / out.bs are filled only where given.
inline void multi_split(const RtCamera& cam, const RtParams& prm, uint32_t n, uint32_t r, const RtAccumState& whole, const RtAccumHalves* hs,
                        const RtAccumBuckets* bs, ShardSnapshot& out) {
    const RtParams p = multi_shard_params(prm, n, r);
    const uint32_t nx = whole.nx, band = p.shard_band, rows = multi_shard_rows(whole.rows, band, n, r);
    const SnapshotHeader h{nx, rows, whole.first_sample, whole.done, accum_frame_id(cam, p)};
    snapshot_header_put(out.st, h);
    out.st.planes = whole.planes, out.st.reserved = 0u;
    out.sum.take(whole.sum, 3u, nx, rows, band, n, r), out.st.sum = out.sum.p.get();
    out.moments.take(whole.moments, 2u, nx, rows, band, n, r), out.st.moments = out.moments.p.get();
    if (whole.planes & RT_ACCUM_STATE_COUNTS) {
        out.counts.take(whole.counts, 1u, nx, rows, band, n, r), out.st.counts = out.counts.p.get();
        out.converged.take(whole.converged, 1u, nx, rows, band, n, r), out.st.converged = out.converged.p.get();
    }
    if (whole.planes & RT_ACCUM_STATE_CHANNELS)
        out.channel_moments.take(whole.channel_moments, 6u, nx, rows, band, n, r), out.st.channel_moments = out.channel_moments.p.get();
    if (hs) {
        snapshot_header_put(out.hs, SnapshotHeader{nx, rows, hs->first_sample, hs->done, h.frame_id});
        for (int k = 0; k < 2; ++k) {
            out.hsum[k].take(hs->sum[k], 3u, nx, rows, band, n, r), out.hs.sum[k] = out.hsum[k].p.get();
            out.hmoments[k].take(hs->moments[k], 2u, nx, rows, band, n, r), out.hs.moments[k] = out.hmoments[k].p.get();
        }
    }
    if (bs) {
        snapshot_header_put(out.bs, SnapshotHeader{nx, rows, bs->first_sample, bs->done, h.frame_id});
        out.bs.M = bs->M, out.bs.reserved = 0u;
        for (uint32_t b = 0; b < bs->M; ++b) out.bsum[b].take(bs->sum[b], 3u, nx, rows, band, n, r), out.bs.sum[b] = out.bsum[b].p.get();
    }
}

} // namespace rt
