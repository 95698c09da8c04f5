// The GPU-free part of the accumulation state and of its snapshots' plane tables (csrc/rt_accum_state.h, rt_accum_planes.h) as a stand-alone program: built with AddressSanitizer + UBSan by
// tests/test_accum_state_host.py and run without a GPU.  It prints one line per section — its name and the number of checks made — and
// "ok"; a failed check prints what failed and ends the program with status 1.  The arrays of every state are exactly as long as the
// scalar fields say, so a check that reads one element too many is an AddressSanitizer report.
#include "rt_accum_planes.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

// accum_state_ref.frame_id of the frames of section "identity" (tests/test_accum_state_host.py recomputes them and compares this text)
#define RT_TEST_ID_BASE 0x386d933fb4ee17eaull
#define RT_TEST_ID_RR 0xf8783b2f08829ec8ull
#define RT_TEST_ID_SHARD 0x60279fb69b84f61cull
#define RT_TEST_ID_SEED 0xc1eeab61c34f8522ull
#define RT_TEST_ID_NEGZERO 0x233afe1c08b4e16aull

static long n_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++n_checks;                                                        \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)
static void section(const char* name) {
    std::printf("%s %ld\n", name, n_checks);
    n_checks = 0;
}

// A well-formed state of nx x rows pixels with the planes `planes`, over vectors of exactly the sizes the header gives.
struct Owned {
    std::vector<float> sum;
    std::vector<double> mom, chm;
    std::vector<uint32_t> cnt;
    std::vector<uint8_t> conv;
    RtAccumState st{};
    Owned(uint32_t nx, uint32_t rows, uint32_t planes, uint32_t done) {
        const size_t npix = (size_t)nx * rows;
        sum.assign(npix * 3, 0.5f), mom.assign(npix * 2, 1.0);
        st.nx = nx, st.rows = rows, st.first_sample = 3u, st.done = done, st.planes = planes, st.reserved = 0u, st.frame_id = 1u;
        // (data() of an empty vector may be NULL: an empty plane still needs a non-NULL pointer)
        static float no_f;
        static double no_d;
        static uint32_t no_u;
        static uint8_t no_b;
        st.sum = npix ? sum.data() : &no_f, st.moments = npix ? mom.data() : &no_d;
        if (planes & RT_ACCUM_STATE_COUNTS) {
            cnt.assign(npix, done), conv.assign(npix, 0u);
            st.counts = npix ? cnt.data() : &no_u, st.converged = npix ? conv.data() : &no_b;
        }
        if (planes & RT_ACCUM_STATE_CHANNELS) {
            chm.assign(npix * 6, 2.0);
            st.channel_moments = npix ? chm.data() : &no_d;
        }
    }
};

// A placed table: every plane aligned to its element behind a 16 B base, no two planes overlapping, none beyond `total`.
static void check_placed(const rt::PlaneTable& t, uint64_t npix, size_t total) {
    for (uint32_t k = 0; k < t.n; ++k) {
        const rt::Plane& p = t.row[k];
        CHECK(p.elem_bytes == 1u || p.elem_bytes == 4u || p.elem_bytes == 12u || p.elem_bytes == 16u);
        CHECK(p.stage % (p.elem_bytes == 16u ? 16u : p.elem_bytes == 1u ? 1u : 4u) == 0u && p.stage + rt::plane_bytes(p, npix) <= total);
        for (uint32_t j = 0; j < k; ++j)
            CHECK(npix == 0u || p.stage + rt::plane_bytes(p, npix) <= t.row[j].stage || t.row[j].stage + rt::plane_bytes(t.row[j], npix) <= p.stage);
    }
}

int main() {
    using namespace rt;
    const uint32_t ALL = RT_ACCUM_STATE_COUNTS | RT_ACCUM_STATE_CHANNELS;
    // ---- states of 0, 1 and 257 pixels, every combination of planes: well formed, and the byte sizes
    const uint32_t shapes[3][2] = {{0u, 0u}, {1u, 1u}, {257u, 1u}};
    for (const auto& sh : shapes)
        for (uint32_t planes = 0; planes <= ALL; ++planes) {
            Owned o(sh[0], sh[1], planes, 7u);
            CHECK(accum_state_invalid(&o.st) == nullptr);
            const uint64_t npix = accum_state_pixels(o.st);
            CHECK(npix == (uint64_t)sh[0] * sh[1]);
            const size_t per = 28u + ((planes & RT_ACCUM_STATE_COUNTS) ? 5u : 0u) + ((planes & RT_ACCUM_STATE_CHANNELS) ? 48u : 0u);
            CHECK(accum_state_pixel_bytes(planes) == per && accum_state_bytes(npix, planes) == npix * per);
            CHECK(o.sum.size() * sizeof(float) == npix * RT_STATE_SUM_BYTES && o.mom.size() * sizeof(double) == npix * RT_STATE_MOMENT_BYTES);
            CHECK(o.chm.size() * sizeof(double) == ((planes & RT_ACCUM_STATE_CHANNELS) ? npix * RT_STATE_CHANNEL_BYTES : 0u));
            // the staging layout of the state's table (rt_accum_planes.h): rows sum, moments[, counts, converged][, channel_moments]
            const bool counts = (planes & RT_ACCUM_STATE_COUNTS) != 0u, channels = (planes & RT_ACCUM_STATE_CHANNELS) != 0u;
            PlaneTable t = state_planes(o.st, counts, channels, nullptr, nullptr, nullptr, nullptr, nullptr);
            CHECK(t.n == 2u + (counts ? 2u : 0u) + (channels ? 1u : 0u) && t.row[0].host == o.st.sum && t.row[1].host == o.st.moments);
            CHECK(planes_place(t, npix) == npix * per);
            check_placed(t, npix, npix * per);
            const size_t sum = t.row[0].stage, moments = t.row[1].stage, after16 = npix * (channels ? 64u : 16u);
            CHECK(moments == 0u && sum == after16);
            if (channels) CHECK(t.row[t.n - 1u].stage == npix * 16u && t.row[t.n - 1u].parts == 3u && t.row[t.n - 1u].elem_bytes == 16u);
            if (counts) CHECK(t.row[2].stage == sum + npix * 12u && t.row[3].stage == t.row[2].stage + npix * 4u && t.row[3].host == o.st.converged);
        }
    { // the halves' and the buckets' tables: the accumulation's own layouts on the local side, placed without a gap in staging
        char* const local = reinterpret_cast<char*>(static_cast<uintptr_t>(1) << 32); // (an address to offset from; nothing is read there)
        for (uint64_t npix : {0ull, 1ull, 255ull, 257ull, 1920ull * 1080ull}) {
            RtAccumHalves hs{};
            PlaneTable t = halves_planes(hs, local, npix);
            const HalvesLayout l = halves_layout(npix);
            CHECK(t.n == 4u && t.row[1].local == local + l.moments[1] && t.row[3].local == local + l.sum[1] && t.row[3].elem_bytes == 12u);
            CHECK(planes_place(t, npix) == l.total);
            check_placed(t, npix, l.total);
            for (uint32_t M : {3u, 16u}) {
                RtAccumBuckets bs{};
                PlaneTable b = buckets_planes(bs, M, local, npix);
                CHECK(b.n == M && b.row[M - 1u].local == local + buckets_plane(npix, M - 1u) && b.row[M - 1u].host == nullptr);
                CHECK(planes_place(b, npix) == buckets_total(npix, M));
                check_placed(b, npix, buckets_total(npix, M));
            }
        }
    }
    { // one mismatch text per field, with the snapshot's noun; what of the window is compared is the caller's choice
        const SnapshotHeader a{8u, 4u, 3u, 7u, 99u};
        CHECK(snapshot_mismatch(a, a, "state", SNAPSHOT_FIRST_AND_DONE).empty());
        SnapshotHeader s = a;
        s.rows = 5u;
        CHECK(snapshot_mismatch(a, s, "halves", SNAPSHOT_ANY_WINDOW) == "nx and rows of the halves are not the accumulation's");
        s = a, s.frame_id = 98u;
        CHECK(snapshot_mismatch(a, s, "state", SNAPSHOT_ANY_WINDOW) == "frame_id of the state is not rt_accum_frame_id of the accumulation's camera and params");
        s = a, s.done = 6u;
        CHECK(snapshot_mismatch(a, s, "state", SNAPSHOT_ANY_WINDOW).empty() && snapshot_mismatch(a, s, "state", SNAPSHOT_FIRST_SAMPLE).empty());
        CHECK(snapshot_mismatch(a, s, "buckets", SNAPSHOT_FIRST_AND_DONE) == "first_sample and done of the buckets are not the accumulation's (rt_accum_import comes first)");
        s = a, s.first_sample = 4u;
        CHECK(snapshot_mismatch(a, s, "state", SNAPSHOT_FIRST_SAMPLE) == "first_sample of the state is not the accumulation's");
        RtAccumBuckets bs{};
        snapshot_header_put(bs, a);
        CHECK(bs.nx == 8u && bs.rows == 4u && bs.first_sample == 3u && bs.done == 7u && bs.frame_id == 99u && snapshot_header(bs).frame_id == 99u);
    }
    CHECK(accum_state_pixel_bytes(ALL) == 81u);
    {
        Owned o(65535u, 0u, 0u, 0u); // a shard without rows
        CHECK(accum_state_invalid(&o.st) == nullptr && accum_state_pixels(o.st) == 0u);
        RtAccumState big{};
        big.nx = 0xFFFFFFFFu, big.rows = 0xFFFFFFFFu;
        CHECK(accum_state_pixels(big) == 0xFFFFFFFFull * 0xFFFFFFFFull); // (no 32-bit product)
    }
    section("sizes");
    // ---- every violated condition of the check, one at a time, on 1 and on 257 pixels
    CHECK(accum_state_invalid(nullptr) != nullptr);
    for (uint32_t nx : {1u, 257u}) {
        const uint32_t last = nx - 1u;
        {
            Owned o(nx, 1u, ALL, 7u);
            o.st.reserved = 1u;
            CHECK(accum_state_invalid(&o.st) != nullptr);
        }
        for (uint32_t bit : {4u, 0x80000000u}) {
            Owned o(nx, 1u, ALL, 7u);
            o.st.planes |= bit;
            CHECK(accum_state_invalid(&o.st) != nullptr);
        }
        {
            Owned o(nx, 1u, 0u, 7u);
            o.st.sum = nullptr;
            CHECK(accum_state_invalid(&o.st) != nullptr);
        }
        {
            Owned o(nx, 1u, 0u, 7u);
            o.st.moments = nullptr;
            CHECK(accum_state_invalid(&o.st) != nullptr);
        }
        { // counts / converged non-NULL exactly when COUNTS is set
            Owned o(nx, 1u, ALL, 7u);
            o.st.counts = nullptr;
            CHECK(accum_state_invalid(&o.st) != nullptr);
            Owned q(nx, 1u, ALL, 7u);
            q.st.converged = nullptr;
            CHECK(accum_state_invalid(&q.st) != nullptr);
            Owned r(nx, 1u, ALL, 7u);
            r.st.planes = RT_ACCUM_STATE_CHANNELS; // the pointers stay
            CHECK(accum_state_invalid(&r.st) != nullptr);
            Owned s(nx, 1u, ALL, 7u);
            s.st.planes = RT_ACCUM_STATE_CHANNELS, s.st.counts = nullptr; // one of the two stays
            CHECK(accum_state_invalid(&s.st) != nullptr);
            s.st.converged = nullptr;
            CHECK(accum_state_invalid(&s.st) == nullptr);
        }
        { // channel_moments non-NULL exactly when CHANNELS is set
            Owned o(nx, 1u, ALL, 7u);
            o.st.channel_moments = nullptr;
            CHECK(accum_state_invalid(&o.st) != nullptr);
            Owned q(nx, 1u, ALL, 7u);
            q.st.planes = RT_ACCUM_STATE_COUNTS;
            CHECK(accum_state_invalid(&q.st) != nullptr);
            q.st.channel_moments = nullptr;
            CHECK(accum_state_invalid(&q.st) == nullptr);
        }
        { // first_sample + done <= 2^32 - 1
            Owned o(nx, 1u, 0u, 7u);
            o.st.first_sample = 0xFFFFFFFFu - 7u;
            CHECK(accum_state_invalid(&o.st) == nullptr);
            o.st.first_sample = 0xFFFFFFFFu - 6u;
            CHECK(accum_state_invalid(&o.st) != nullptr);
            o.st.first_sample = 0xFFFFFFFFu, o.st.done = 0xFFFFFFFFu;
            CHECK(accum_state_invalid(&o.st) != nullptr);
            o.st.first_sample = 0u;
            CHECK(accum_state_invalid(&o.st) == nullptr);
        }
        { // the invariant of the counts, on the last pixel (the first is the same code)
            Owned o(nx, 1u, RT_ACCUM_STATE_COUNTS, 7u);
            o.conv[last] = 2u;
            CHECK(accum_state_invalid(&o.st) != nullptr);
            o.conv[last] = 255u;
            CHECK(accum_state_invalid(&o.st) != nullptr);
            o.conv[last] = 1u; // converged with every sample: allowed (it stopped at the last decision)
            CHECK(accum_state_invalid(&o.st) == nullptr);
            o.cnt[last] = 4u; // converged earlier
            CHECK(accum_state_invalid(&o.st) == nullptr);
            o.cnt[last] = 8u; // more than were issued
            CHECK(accum_state_invalid(&o.st) != nullptr);
            o.conv[last] = 0u;
            CHECK(accum_state_invalid(&o.st) != nullptr);
            o.cnt[last] = 6u; // active and short of a sample
            CHECK(accum_state_invalid(&o.st) != nullptr);
            o.cnt[last] = 7u;
            CHECK(accum_state_invalid(&o.st) == nullptr);
            o.cnt[0] = nx > 1u ? 0u : 7u, o.conv[0] = nx > 1u ? 1u : 0u; // a pixel that never got a sample, converged: within the invariant
            CHECK(accum_state_invalid(&o.st) == nullptr);
        }
        { // the values are not judged: NaN, inf and negative sums are a state like any other
            Owned o(nx, 1u, ALL, 7u);
            o.sum[0] = std::numeric_limits<float>::quiet_NaN(), o.mom[1] = std::numeric_limits<double>::infinity(), o.chm[5] = -1.0;
            CHECK(accum_state_invalid(&o.st) == nullptr);
        }
    }
    section("check");
    // ---- the identity: constants that tests/accum_state_ref.py produced (FNV-1a 64 over the bytes the header lists)
    {
        RtCamera cam{};
        const float c12[12] = {13.0f, 2.0f, 3.0f, 4.5f, 0.0f, -1.25f, 0.0f, 2.25f, 0.0f, -2.0f, -1.0f, 0.5f};
        for (int k = 0; k < 3; ++k)
            cam.origin[k] = c12[k], cam.horizontal[k] = c12[3 + k], cam.vertical[k] = c12[6 + k], cam.lower_left_corner[k] = c12[9 + k];
        RtParams p{};
        p.nx = 40u, p.ny = 20u, p.spp = 7u, p.max_depth = 50, p.seed = 1234u;
        const uint64_t base = accum_frame_id(cam, p);
        CHECK(base == RT_TEST_ID_BASE);
        // what does not enter
        RtParams q = p;
        q.spp = 1000u, q.spp_slice = 3u, q.flags = RT_FLAG_BRUTE_FORCE | 4u | 8u, q.reserved = 0u;
        CHECK(accum_frame_id(cam, q) == base);
        q = p, q.shard_count = 1u, q.shard_band = 9u, q.shard_id = 5u; // shard_count <= 1: (0, 1, 0) however it was written
        CHECK(accum_frame_id(cam, q) == base);
        q.shard_count = 0u;
        CHECK(accum_frame_id(cam, q) == base);
        // what does
        q = p, q.flags = RT_FLAG_RUSSIAN_ROULETTE | RT_FLAG_BRUTE_FORCE;
        CHECK(accum_frame_id(cam, q) == RT_TEST_ID_RR);
        q = p, q.shard_count = 2u, q.shard_band = 4u, q.shard_id = 1u;
        CHECK(accum_frame_id(cam, q) == RT_TEST_ID_SHARD);
        q = p, q.seed = 0xFEDCBA9876543210ull, q.max_depth = -1;
        CHECK(accum_frame_id(cam, q) == RT_TEST_ID_SEED);
        RtCamera neg = cam;
        neg.horizontal[1] = -0.0f; // a bit pattern, not a value: -0 is another frame
        CHECK(accum_frame_id(neg, p) == RT_TEST_ID_NEGZERO && accum_frame_id(neg, p) != base);
        q = p, q.nx = 20u, q.ny = 40u;
        CHECK(accum_frame_id(cam, q) != base);
        // the empty hash is the offset basis, one zero byte the first step
        Fnv1a64 f;
        CHECK(f.h == 0xcbf29ce484222325ull);
        f.byte(0u);
        CHECK(f.h == 0xaf63bd4c8601b7dfull);
    }
    section("identity");
    std::printf("ok\n");
    return 0;
}
