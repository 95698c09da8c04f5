// rt_accum_planes.h — the GPU-free description of what rt_accum_export / _import / _merge and their _halves and _buckets twins move: the
// per-pixel planes of a snapshot (an RtAccumState, RtAccumHalves or RtAccumBuckets) between the accumulation's local pixel order and the
// caller's arrays in image order, through one staging buffer.  A snapshot is a table of planes; k_planes_move (rt_accum_state_kernels.h)
// and the two host paths of rt_api.hip (planes_to_host, planes_from_host) know tables only, so another tracked quantity is a few more rows.
// Like rt_halves_plan.h: no context, no device call, plain values in and out; tests/accum_state_main.cpp, halves_plan_main.cpp and
// buckets_plan_main.cpp run it under AddressSanitizer + UBSan without a GPU.
#pragma once
#include "rt_accum_state.h"
#include "rt_buckets_plan.h"
#include "rt_features_plan.h"
#include "rt_filter_plan.h"
#include "rt_halves_plan.h"

#include <string>

namespace rt {

// One plane: `elem_bytes` (1, 4, 12 or 16) per pixel and part.  `parts` is 1, or 3 for the channel moments: local part k lies
// k * npix * elem_bytes behind `local`; in image order the parts of a pixel lie side by side, part k at k * elem_bytes into a group of
// parts * elem_bytes.
struct Plane {
    void* host;          // the caller's array, image order (NULL on export: not asked for; an import never writes through it)
    void* local;         // the accumulation's plane on the device, local pixel order
    size_t stage;        // where the plane lies in the staging buffer, image order (planes_place)
    uint32_t elem_bytes;
    uint32_t parts;
};
constexpr uint32_t RT_PLANES_MAX = 16u; // the buckets need the most rows; the state at most 5, the halves 4
static_assert(RT_PLANES_MAX == RT_BUCKETS_MAX, "a PlaneTable holds one row per bucket");
struct PlaneTable {
    uint32_t n;
    Plane row[RT_PLANES_MAX];
};
inline void planes_push(PlaneTable& t, const void* host, void* local, uint32_t elem_bytes, uint32_t parts = 1u) {
    t.row[t.n++] = Plane{const_cast<void*>(host), local, 0u, elem_bytes, parts};
}
inline size_t plane_bytes(const Plane& p, uint64_t npix) { return (size_t)npix * p.elem_bytes * p.parts; }

// Gives every row its place in one staging buffer of npix pixels and returns the buffer's size: the 16 B elements first, then the 12 B
// and 4 B ones, then the bytes, each group in table order, so that every plane keeps the alignment of its element (16, 4, 4, 1) behind
// a base aligned to 16 B.
inline size_t planes_place(PlaneTable& t, uint64_t npix) {
    size_t off = 0;
    for (const uint32_t align : {16u, 4u, 1u})
        for (uint32_t k = 0; k < t.n; ++k) {
            Plane& p = t.row[k];
            if ((p.elem_bytes % 16u == 0u ? 16u : p.elem_bytes % 4u == 0u ? 4u : 1u) == align) p.stage = off, off += plane_bytes(p, npix);
        }
    return off;
}

// ---- the three snapshots as tables ------------------------------------------------------------------------------------------------------
// sum, moments, then counts and converged (`counts`), then channel_moments (`channels`); the five local planes as rt_api.hip holds them.
inline PlaneTable state_planes(const RtAccumState& st, bool counts, bool channels, void* sum, void* mom, void* cnt, void* flag, void* chm) {
    PlaneTable t{};
    planes_push(t, st.sum, sum, RT_STATE_SUM_BYTES);
    planes_push(t, st.moments, mom, RT_STATE_MOMENT_BYTES);
    if (counts) planes_push(t, st.counts, cnt, RT_STATE_COUNT_BYTES), planes_push(t, st.converged, flag, RT_STATE_FLAG_BYTES);
    if (channels) planes_push(t, st.channel_moments, chm, RT_STATE_CHANNEL_BYTES / 3u, 3u);
    return t;
}
// `local`: the accumulation's buffer of halves (halves_layout over npix pixels)
inline PlaneTable halves_planes(const RtAccumHalves& hs, void* local, uint64_t npix) {
    const HalvesLayout l = halves_layout(npix);
    PlaneTable t{};
    for (int h = 0; h < 2; ++h) planes_push(t, hs.moments[h], (char*)local + l.moments[h], RT_HALVES_MOMENT_BYTES);
    for (int h = 0; h < 2; ++h) planes_push(t, hs.sum[h], (char*)local + l.sum[h], RT_HALVES_SUM_BYTES);
    return t;
}
// `local`: the accumulation's buffer of M <= RT_BUCKETS_MAX buckets (buckets_plane over npix pixels)
inline PlaneTable buckets_planes(const RtAccumBuckets& bs, uint32_t M, void* local, uint64_t npix) {
    PlaneTable t{};
    for (uint32_t b = 0; b < M; ++b) planes_push(t, bs.sum[b], (char*)local + buckets_plane(npix, b), RT_BUCKETS_SUM_BYTES);
    return t;
}

// `local`: the accumulation's filter plane (behind the table in its buffer: rt_filter_plan.h)
inline PlaneTable filter_planes(const RtAccumFilter& fs, void* local) {
    PlaneTable t{};
    planes_push(t, fs.plane, local, RT_FILTER_PIXEL_BYTES);
    return t;
}

// `local`: the accumulation's feature records, four quarter planes of 16 B (rt_features_plan.h); in image order a pixel's quarters lie side
// by side: the 64 B RtFeaturePixel
inline PlaneTable features_planes(const RtAccumFeatures& fs, void* local) {
    PlaneTable t{};
    planes_push(t, fs.plane, local, RT_FEATURES_QUARTER_BYTES, RT_FEATURES_QUARTERS);
    return t;
}

// ---- the scalar fields the three snapshots share ----------------------------------------------------------------------------------------
struct SnapshotHeader {
    uint32_t nx, rows, first_sample, done;
    uint64_t frame_id;
};
template <class S>
SnapshotHeader snapshot_header(const S& s) {
    return SnapshotHeader{s.nx, s.rows, s.first_sample, s.done, s.frame_id};
}
template <class S>
void snapshot_header_put(S& s, const SnapshotHeader& h) {
    s.nx = h.nx, s.rows = h.rows, s.first_sample = h.first_sample, s.done = h.done, s.frame_id = h.frame_id;
}
// What an import or a merge asks of a well-formed snapshot `s` ("the state", "the halves", "the buckets": `noun`) against the open
// accumulation `a`: empty, or the mismatch.  `window`: what of the sample window must agree as well.
enum SnapshotWindow { SNAPSHOT_ANY_WINDOW, SNAPSHOT_FIRST_SAMPLE, SNAPSHOT_FIRST_AND_DONE };
inline std::string snapshot_mismatch(const SnapshotHeader& a, const SnapshotHeader& s, const char* noun, SnapshotWindow window) {
    const std::string of = std::string(" of the ") + noun;
    if (s.nx != a.nx || s.rows != a.rows) return "nx and rows" + of + " are not the accumulation's";
    if (s.frame_id != a.frame_id) return "frame_id" + of + " is not rt_accum_frame_id of the accumulation's camera and params";
    if (window == SNAPSHOT_FIRST_SAMPLE && s.first_sample != a.first_sample) return "first_sample" + of + " is not the accumulation's";
    if (window == SNAPSHOT_FIRST_AND_DONE && (s.first_sample != a.first_sample || s.done != a.done))
        return "first_sample and done" + of + " are not the accumulation's (rt_accum_import comes first)";
    return std::string();
}

} // namespace rt
