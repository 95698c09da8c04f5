// rt_multi_accum.h — "Progressive accumulation across devices" of include/rtow_mi355x.h (included behind rt_multi.h at the end of rt_api.hip).
//
// Device i holds an ordinary accumulation (rt_accum_*) over shard (band, n, i) of the frame; the same add runs on every device, one host
// thread each, so the shards stay in lock-step.  The adaptive decision is per pixel, so nothing is exchanged while sampling.  What the
// filters and the frame figures need is the frame in one piece: rt_multi_accum_join brings EVERY plane of every shard to the first device,
// device to device, and installs it in a whole-frame accumulation there — the mirror, a context of its own that never traces:
//
//   1. device i: k_planes_move<true> (rt_accum_state_kernels.h, unchanged) writes the shard's state, halves and buckets tables into one
//      send buffer in the shard's image order, the tables one behind the other (rt_multi_accum_plan.h: multi_place)
//   2. one gather into n slots of equal stride on the first device: device-to-device copies with one event each
//      (RT_MULTI_COPY_GATHER) or one group of ncclSend / ncclRecv in bytes — the two mechanisms of rt_multi_render
//   3. first device: k_planes_join, once per shard and table, moves a slot's rows to where the mirror's local pixel order keeps them
//
// A shard without rows sends nothing.  There is no host staging.  k_planes_join is in no variant table and no ledger family.
#pragma once
#include "rt_multi_accum_plan.h"

namespace rt {

// One thread per pixel of shard r in slot order p = lj * nx + i; the pixel is (i, j) of the frame with j = multi_image_row(lj).  Every row
// of the table moves as k_planes_move<false> moves it — a load and a store of the element's own width, bit for bit — except that the
// local side is the WHOLE frame's: the pixel's index is local_of_pixel of the mirror's order at (i, j) and the parts of a plane lie
// frame_npix elements apart, while on the slot side they lie side by side.
__global__ __launch_bounds__(256) void k_planes_join(PlaneTable t, char* slot, uint32_t nx, uint32_t rows, uint32_t band, uint32_t n_shards, uint32_t r,
                                                     uint32_t tiles_per_row, uint32_t tile_pixels, uint32_t frame_npix) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nx * rows) return;
    const uint32_t lj = p / nx, i = p - lj * nx;
    const uint32_t j = n_shards > 1u ? ((lj / band) * n_shards + r) * band + lj % band : lj;
    const size_t ap = local_of_pixel(nx, tiles_per_row, tile_pixels, i, j);
    for (uint32_t k = 0; k < t.n; ++k) {
        const Plane pl = t.row[k];
        char *local = static_cast<char*>(pl.local), *image = slot + pl.stage;
        if (pl.elem_bytes == 16u && pl.parts == 3u) {
            plane_move_three<false>(reinterpret_cast<uint4*>(local) + ap, reinterpret_cast<uint4*>(image) + 3 * (size_t)p, frame_npix);
            continue;
        }
        for (uint32_t part = 0; part < pl.parts; ++part) {
            const size_t lp = (size_t)part * frame_npix + ap, ip = (size_t)p * pl.parts + part;
            switch (pl.elem_bytes) {
            case 1u: plane_move<false, uint8_t>(local, image, lp, ip); break;
            case 4u: plane_move<false, uint32_t>(local, image, lp, ip); break;
            case 12u: plane_move<false, StateRgb>(local, image, lp, ip); break;
            default: plane_move<false, uint4>(local, image, lp, ip); break;
            }
        }
    }
}

} // namespace rt

namespace {

// `work(i)` for every device, one host thread per device (as rt_multi_render does it), all finished on return
template <class Work>
void multi_each(uint32_t n, Work work) {
    if (n == 1u) return work(0u);
    std::vector<std::thread> th;
    for (uint32_t i = 0; i < n; ++i) th.emplace_back(work, i);
    for (auto& t : th) t.join();
}

int multi_accum_require_open(RtMulti* m, const char* who) {
    if (m->accum.broken) return multi_fail(m, RT_ERR_STATE, std::string(who) + ": the accumulation was ended by a failure (" + m->accum.why + "); rt_multi_accum_begin starts another");
    return m->accum.open ? RT_OK : multi_fail(m, RT_ERR_STATE, std::string(who) + ": no accumulation begun (or it was ended: rtow_mi355x.h)");
}

void multi_accum_close(RtMulti* m) {
    for (RtCtx* c : m->ctx) (void)rt_accum_end(c);
    if (m->mirror) m->mirror->accum.open = false;
    m->accum.open = false;
}

// What the same call answered on every device.  All RT_OK: RT_OK.  The same refusal of the arguments or the state everywhere (`refused`
// says a device changed nothing before it answered): that code with the first device's text, and the accumulation is as it was.  Anything
// else: the shards no longer belong together — the accumulation ends on every device and the error names the one that failed.
int multi_accum_settle(RtMulti* m, const char* who, const std::vector<int>& rcs, bool refused = true) {
    size_t bad = rcs.size();
    bool same = true;
    for (size_t i = 0; i < rcs.size(); ++i) {
        if (rcs[i] && bad == rcs.size()) bad = i;
        same = same && rcs[i] == rcs[0];
    }
    if (bad == rcs.size()) return RT_OK;
    const int rc = rcs[bad];
    const std::string why = std::string("device ") + std::to_string(m->devices[bad]) + ": " + rt_last_error(m->ctx[bad]);
    if (refused && same && (rc == RT_ERR_INVALID || rc == RT_ERR_STATE || rc == RT_ERR_UNSUPPORTED)) return multi_fail(m, rc, why);
    multi_accum_close(m);
    m->accum.broken = true, m->accum.why = why;
    return multi_fail(m, rc, std::string(who) + ": " + why + " (the accumulation has ended on every device)");
}

int multi_accum_add(RtMulti* m, const char* who, uint32_t n_samples, bool adaptive, const RtAdaptive* ad, RtStats* stats) {
    if (!m) return RT_ERR_INVALID;
    if (const int rc = multi_accum_require_open(m, who)) return rc;
    const uint32_t n = (uint32_t)m->ctx.size();
    std::vector<int> rcs(n, RT_OK);
    std::vector<RtStats> sts(n);
    multi_each(n, [&](uint32_t i) {
        rcs[i] = adaptive ? rt_accum_add_adaptive(m->ctx[i], n_samples, ad, &sts[i]) : rt_accum_add(m->ctx[i], n_samples, &sts[i]);
    });
    if (const int rc = multi_accum_settle(m, who, rcs)) return rc;
    if (stats) multi_sum_stats(sts, stats);
    return RT_OK;
}

MultiTracked multi_tracked(const RtCtx::Accum& a) { return MultiTracked{a.adaptive, a.channels, a.halves, a.buckets}; }
// The tables over the planes of `c`'s accumulation (the open one, or the mirror's being installed): npix = the pixels its planes hold
MultiTables multi_tables_of(RtCtx* c, const MultiTracked& tr, uint64_t npix) {
    return multi_tables(tr, c->accum_sum.p, c->accum_mom.p, c->accum_cnt.p, c->accum_flag.p, c->accum_chm.p, c->accum_halves.p, c->accum_buckets.p, npix);
}

} // namespace

extern "C" {

int rt_multi_accum_begin(RtMulti* m, const RtCamera* cam, const RtParams* params, uint32_t first_sample, uint32_t track, uint32_t M) {
    if (!m) return RT_ERR_INVALID;
    if (!cam || !params) return multi_fail(m, RT_ERR_INVALID, "rt_multi_accum_begin: camera/params NULL");
    if (track & RT_MULTI_UNSUPPORTED_FEATURES)
        return multi_fail(m, RT_ERR_UNSUPPORTED, "rt_multi_accum_begin: RT_MULTI_UNSUPPORTED_FEATURES: first-hit features of shards are not covered (rtow_mi355x.h \"First-hit features\")");
    if (track & ~(RT_MULTI_TRACK_CHANNELS | RT_MULTI_TRACK_HALVES | RT_MULTI_TRACK_BUCKETS))
        return multi_fail(m, RT_ERR_INVALID, "rt_multi_accum_begin: track holds a bit that is no RT_MULTI_TRACK_*");
    if ((track & RT_MULTI_TRACK_BUCKETS) && (M < RT_BUCKETS_MIN || M > RT_BUCKETS_MAX))
        return multi_fail(m, RT_ERR_INVALID, "rt_multi_accum_begin: M must be 3 .. RT_BUCKETS_MAX with RT_MULTI_TRACK_BUCKETS");
    const uint32_t n = (uint32_t)m->ctx.size();
    if (!m->mirror) { // a context of the first device that holds the joined accumulation and never traces: no scene, no work buffers
        const int rc = rt_ctx_create(m->devices[0], &m->mirror);
        if (rc) return multi_fail(m, rc, std::string("rt_multi_accum_begin: the joined context: ") + rt_last_error(nullptr));
        m->mirror->accum.mirror = true;
        m->send.resize(n);
    }
    multi_accum_close(m);
    m->accum.broken = false, m->accum.why.clear();
    RtMulti::Accum& a = m->accum;
    a.cam = *cam, a.prm = *params, a.first = first_sample, a.band = multi_band(params->shard_band);
    a.prm.shard_band = a.band, a.prm.shard_count = 1u, a.prm.shard_id = 0u;
    std::vector<int> rcs(n, RT_OK);
    multi_each(n, [&](uint32_t i) {
        RtCtx* c = m->ctx[i];
        const RtParams p = multi_shard_params(a.prm, n, i);
        int rc = rt_accum_begin(c, cam, &p, first_sample);
        if (!rc && (track & RT_MULTI_TRACK_CHANNELS)) rc = rt_accum_track_channels(c);
        if (!rc && (track & RT_MULTI_TRACK_HALVES)) rc = rt_accum_track_halves(c);
        if (!rc && (track & RT_MULTI_TRACK_BUCKETS)) rc = rt_accum_track_buckets(c, M);
        rcs[i] = rc;
    });
    for (uint32_t i = 0; i < n; ++i)
        if (rcs[i]) {
            const std::string why = std::string("device ") + std::to_string(m->devices[i]) + ": " + rt_last_error(m->ctx[i]);
            multi_accum_close(m);
            return multi_fail(m, rcs[i], why);
        }
    a.open = true;
    return RT_OK;
}

int rt_multi_accum_add(RtMulti* m, uint32_t n_samples, RtStats* stats) { return multi_accum_add(m, "rt_multi_accum_add", n_samples, false, nullptr, stats); }
int rt_multi_accum_add_adaptive(RtMulti* m, uint32_t n_samples, const RtAdaptive* ad, RtStats* stats) {
    return multi_accum_add(m, "rt_multi_accum_add_adaptive", n_samples, true, ad, stats);
}

int rt_multi_accum_import(RtMulti* m, const RtAccumState* st, const RtAccumHalves* hs, const RtAccumBuckets* bs) {
    if (!m) return RT_ERR_INVALID;
    const char* who = "rt_multi_accum_import";
    if (const int rc = multi_accum_require_open(m, who)) return rc;
    const RtMulti::Accum& a = m->accum;
    const auto invalid = [&](const std::string& why) { return multi_fail(m, RT_ERR_INVALID, std::string(who) + ": " + why); };
    // the whole-frame snapshot against the whole frame, before any device is touched
    if (const char* why = accum_state_invalid(st)) return invalid(why);
    SnapshotHeader whole{a.prm.nx, a.prm.ny, a.first, st->done, accum_frame_id(a.cam, a.prm)};
    std::string why = snapshot_mismatch(whole, snapshot_header(*st), "state", SNAPSHOT_FIRST_SAMPLE);
    if (why.empty() && hs) {
        if (const char* w = accum_halves_invalid(hs)) return invalid(w);
        why = snapshot_mismatch(whole, snapshot_header(*hs), "halves", SNAPSHOT_FIRST_AND_DONE);
    }
    if (why.empty() && bs) {
        if (const char* w = accum_buckets_invalid(bs)) return invalid(w);
        why = snapshot_mismatch(whole, snapshot_header(*bs), "buckets", SNAPSHOT_FIRST_AND_DONE);
    }
    if (!why.empty()) return invalid(why);
    const uint32_t n = (uint32_t)m->ctx.size();
    std::vector<int> rcs(n, RT_OK);
    std::vector<int> changed(n, 0); // the state is in: a refusal behind it leaves that device apart from the others
    multi_each(n, [&](uint32_t i) {
        ShardSnapshot s; // the split is host work: one shard's rows at a time per thread
        multi_split(a.cam, a.prm, n, i, *st, hs, bs, s);
        int rc = rt_accum_import(m->ctx[i], &s.st);
        if (!rc) changed[i] = 1;
        if (!rc && hs) rc = rt_accum_import_halves(m->ctx[i], &s.hs);
        if (!rc && bs) rc = rt_accum_import_buckets(m->ctx[i], &s.bs);
        rcs[i] = rc;
    });
    return multi_accum_settle(m, who, rcs, std::none_of(changed.begin(), changed.end(), [](int c) { return c != 0; }));
}

int rt_multi_accum_join(RtMulti* m, RtCtx** joined) {
    if (!m) return RT_ERR_INVALID;
    const char* who = "rt_multi_accum_join";
    if (!joined) return multi_fail(m, RT_ERR_INVALID, "rt_multi_accum_join: joined is NULL");
    *joined = m->mirror;
    if (const int rc = multi_accum_require_open(m, who)) return rc;
    const RtMulti::Accum& a = m->accum;
    RtCtx* const mir = m->mirror;
    RtCtx* const c0 = m->ctx[0];
    const uint32_t n = (uint32_t)m->ctx.size(), nx = a.prm.nx, ny = a.prm.ny, band = a.band;
    const RtCtx::Accum lead = c0->accum; // the shards are in lock-step: what the first one says of done and of the tracking holds for all
    for (uint32_t i = 0; i < n; ++i) {
        const RtCtx::Accum& s = m->ctx[i]->accum;
        if (!s.open || s.done != lead.done || s.adaptive != lead.adaptive || s.channels != lead.channels || s.halves != lead.halves || s.buckets != lead.buckets ||
            s.nx != nx || s.rows != multi_shard_rows(ny, band, n, i))
            return multi_fail(m, RT_ERR_STATE, std::string(who) + ": device " + std::to_string(m->devices[i]) +
                                                   ": its accumulation is not the shard begun here (a call on the context itself ended or changed it)");
    }
    const MultiTracked tr = multi_tracked(lead);
    const uint32_t npix = nx * ny;
    const size_t stride = multi_slot_stride(tr, nx, multi_rows_pad(ny, band, n));
    mir->accum.open = false; // (until every pixel is rewritten)
    // ---- the mirror's planes and the slots, on the first device (plain hipMalloc for what other devices address) ----------------------
    const auto first_fail = [&](int rc) { return multi_fail(m, rc, std::string(who) + ": " + rt_last_error(mir)); };
    int rc;
    if (hipSetDevice(m->devices[0]) != hipSuccess) return multi_fail(m, RT_ERR_DEVICE, "hipSetDevice failed");
    const PixelOrder po = pixel_order(0u, scene_is_general(c0), nx, ny); // what one context with this scene and default options picks
    {
        const uint32_t nb = (npix + 255u) / 256u;
        if ((rc = ensure(mir, mir->accum_sum, (size_t)npix * 3 * sizeof(float)))) return first_fail(rc);
        if ((rc = ensure(mir, mir->accum_mom, (size_t)npix * sizeof(double2)))) return first_fail(rc);
        if ((rc = ensure(mir, mir->accum_partials, (size_t)nb * sizeof(double2) + 3 * sizeof(double)))) return first_fail(rc);
        if (!mir->h_noise && hipHostMalloc((void**)&mir->h_noise, 3 * sizeof(double), hipHostMallocDefault) != hipSuccess)
            return multi_fail(m, RT_ERR_NOMEM, std::string(who) + ": hipHostMalloc failed");
        if (tr.counts && (rc = ensure_adaptive(mir, npix))) return first_fail(rc);
        if (tr.channels && (rc = ensure_channels(mir, npix))) return first_fail(rc);
        if (tr.halves && (rc = ensure_halves(mir, npix))) return first_fail(rc);
        if (tr.buckets && (rc = ensure_buckets(mir, npix, tr.buckets))) return first_fail(rc);
        if ((rc = ensure(mir, m->slots, stride * n, true))) return first_fail(rc);
    }
    // ---- 1. every shard's tables into its send buffer, image order of the shard --------------------------------------------------------
    std::vector<size_t> bytes(n, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        RtCtx* c = m->ctx[i];
        const uint32_t np = c->accum.npix;
        if (np == 0u) continue; // a shard without rows sends nothing
        if (hipSetDevice(m->devices[i]) != hipSuccess) return multi_fail(m, RT_ERR_DEVICE, "hipSetDevice failed");
        MultiTables mt = multi_tables_of(c, tr, np);
        bytes[i] = multi_place(mt, np);
        if ((rc = ensure(c, m->send[i], bytes[i], true))) return multi_fail(m, rc, std::string("device ") + std::to_string(m->devices[i]) + ": " + rt_last_error(c));
        for (uint32_t k = 0; k < RT_MULTI_TABLES; ++k)
            if (mt.t[k].n) launch_planes_move(c, mt.t[k], m->send[i].as<char>() + mt.base[k], true);
        if (hipGetLastError() != hipSuccess) return multi_fail(m, RT_ERR_DEVICE, std::string(who) + ": k_planes_move could not be launched");
    }
    // ---- 2. the one exchange step: send buffer i to slot i of the first device ----------------------------------------------------------
    char* const slots = m->slots.as<char>();
    if (m->copy_gather) {
        hipError_t e = hipSuccess;
        for (uint32_t i = 0; i < n && e == hipSuccess; ++i) {
            e = hipSetDevice(m->devices[i]);
            if (e == hipSuccess && bytes[i]) e = hipMemcpyAsync(slots + i * stride, m->send[i].p, bytes[i], hipMemcpyDeviceToDevice, m->ctx[i]->stream);
            if (e == hipSuccess) e = hipEventRecord(m->gather_done[i], m->ctx[i]->stream);
        }
        if (e == hipSuccess) e = hipSetDevice(m->devices[0]);
        for (uint32_t k = 1; k < n && e == hipSuccess; ++k) e = hipStreamWaitEvent(c0->stream, m->gather_done[k], 0);
        if (e != hipSuccess) return multi_fail(m, RT_ERR_DEVICE, std::string(who) + ": copy gather: " + hipGetErrorString(e));
    } else {
        // as rt_multi_render: the first device's own buffer is a local copy, the others send and the first posts the matching receives in
        // one group; counts are bytes.  (The group is UNVERIFIED ON HARDWARE for n > 1, as rt_multi_create says of every RCCL step.)
        if (hipSetDevice(m->devices[0]) != hipSuccess ||
            (bytes[0] && hipMemcpyAsync(slots, m->send[0].p, bytes[0], hipMemcpyDeviceToDevice, c0->stream) != hipSuccess))
            return multi_fail(m, RT_ERR_DEVICE, std::string(who) + ": copy of the first device's own planes failed");
        if (n > 1u) {
            ncclResult_t nr = m->GroupStart();
            for (uint32_t i = 1; i < n && nr == ncclSuccess; ++i) {
                if (bytes[i] == 0u) continue;
                if (hipSetDevice(m->devices[i]) != hipSuccess) return multi_fail(m, RT_ERR_DEVICE, "hipSetDevice failed");
                nr = m->Send(m->send[i].p, bytes[i], ncclUint8, 0, m->comms[i], m->ctx[i]->stream);
                if (nr == ncclSuccess && hipSetDevice(m->devices[0]) != hipSuccess) return multi_fail(m, RT_ERR_DEVICE, "hipSetDevice failed");
                if (nr == ncclSuccess) nr = m->Recv(slots + i * stride, bytes[i], ncclUint8, (int)i, m->comms[0], c0->stream);
            }
            const ncclResult_t ne = m->GroupEnd();
            if (nr == ncclSuccess) nr = ne;
            if (nr != ncclSuccess) return multi_fail(m, RT_ERR_DEVICE, std::string(who) + ": ncclSend / ncclRecv: " + m->GetErrorString(nr));
        }
    }
    // ---- 3. every slot into the mirror's local pixel order, on the first context's stream behind the gather -----------------------------
    if (hipSetDevice(m->devices[0]) != hipSuccess) return multi_fail(m, RT_ERR_DEVICE, "hipSetDevice failed");
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t rows = m->ctx[i]->accum.rows, np = m->ctx[i]->accum.npix;
        if (np == 0u) continue;
        MultiTables jt = multi_tables_of(mir, tr, npix); // local side: the planes of the whole frame; slot side: placed for the shard's pixels
        (void)multi_place(jt, np);
        for (uint32_t k = 0; k < RT_MULTI_TABLES; ++k)
            if (jt.t[k].n)
                hipLaunchKernelGGL(k_planes_join, dim3((np + 255u) / 256u), dim3(256), 0, c0->stream, jt.t[k], slots + i * stride + jt.base[k], nx, rows, band, n, i,
                                   po.tiles_per_row, po.tile_pixels, npix);
    }
    hipError_t e = hipGetLastError();
    for (uint32_t i = 0; i < n && e == hipSuccess; ++i) // every device's part has finished: the mirror is read on its own stream from here on
        if ((e = hipSetDevice(m->devices[i])) == hipSuccess) e = hipStreamSynchronize(m->ctx[i]->stream);
    if (e != hipSuccess) return multi_fail(m, RT_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    RtCtx::Accum j{};
    j.cam = a.cam, j.prm = a.prm, j.first = a.first, j.done = lead.done;
    j.nx = nx, j.rows = ny, j.npix = npix, j.tiles_per_row = po.tiles_per_row, j.tile_pixels = po.tile_pixels;
    j.adaptive = lead.adaptive, j.channels = lead.channels, j.halves = lead.halves, j.buckets = lead.buckets;
    j.added = true, j.mirror = true, j.open = true;
    mir->accum = j;
    return RT_OK;
}

int rt_multi_accum_end(RtMulti* m) {
    if (!m) return RT_ERR_INVALID;
    multi_accum_close(m);
    m->accum.broken = false, m->accum.why.clear();
    return RT_OK;
}

} // extern "C"
