// The GPU-free part of rt_multi_accum_* (csrc/rt_multi_accum_plan.h) as a stand-alone program: built with AddressSanitizer + UBSan by
// tests/test_multi_accum_host.py and run without a GPU.  It prints one line per section — its name and the number of checks made — and
// "ok"; a failed check prints what failed and ends the program with status 1.  The arrays of every snapshot, whole or split, are exactly
// as long as the scalar fields say, so a split that reads or writes one element too many is an AddressSanitizer report.
#include "rt_multi_accum_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace rt;

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

static const uint32_t SIZES[][2] = {{1, 1}, {7, 3}, {16, 11}, {24, 27}, {1920, 1080}};
static const uint32_t BANDS[] = {1, 4, 8}, COUNTS[] = {1, 2, 3, 8};

// Every image row is owned by exactly one (shard, local row); local rows ascend with image rows; the padded row count is the largest.
static void row_map() {
    for (const auto& sz : SIZES)
        for (const uint32_t band : BANDS)
            for (const uint32_t n : COUNTS) {
                const uint32_t ny = sz[1];
                std::vector<uint32_t> owners(ny, 0u);
                uint32_t total = 0, most = 0;
                for (uint32_t r = 0; r < n; ++r) {
                    const uint32_t rows = multi_shard_rows(ny, band, n, r);
                    total += rows, most = rows > most ? rows : most;
                    uint32_t before = 0;
                    for (uint32_t lj = 0; lj < rows; ++lj) {
                        const uint32_t j = multi_image_row(lj, band, n, r);
                        CHECK(j < ny);
                        CHECK(lj == 0u || j > before);
                        CHECK(n == 1u ? j == lj : (j / band) % n == r);
                        before = j, ++owners[j];
                    }
                    CHECK(multi_image_row(rows, band, n, r) >= ny); // the shard ends where the frame does
                }
                CHECK(total == ny);
                for (uint32_t j = 0; j < ny; ++j) CHECK(owners[j] == 1u);
                CHECK(multi_rows_pad(ny, band, n) == most);
                CHECK(multi_shard_rows(ny, band, n, n) == (n == 1u ? ny : 0u));
            }
    CHECK(multi_band(0u) == 8u && multi_band(1u) == 1u && multi_band(5u) == 5u);
    section("row_map");
}

// The tables of a shard in its buffer: bases aligned to 16 B, every plane aligned to its element, no two planes overlapping, all inside
// the buffer, and the buffer inside the slot stride — for every plane set.
static void placement() {
    const MultiTracked SETS[] = {{false, false, false, 0u}, {true, false, false, 0u}, {false, true, false, 0u}, {true, true, false, 0u},
                                 {false, false, true, 0u},  {false, false, false, 3u}, {true, true, true, 3u},  {true, true, true, 16u}};
    for (const auto& sz : SIZES)
        for (const uint32_t band : BANDS)
            for (const uint32_t n : COUNTS)
                for (const MultiTracked& tr : SETS) {
                    const uint32_t nx = sz[0], ny = sz[1];
                    const size_t stride = multi_slot_stride(tr, nx, multi_rows_pad(ny, band, n));
                    CHECK(stride % 16u == 0u);
                    for (uint32_t r = 0; r < n; ++r) {
                        const uint64_t npix = (uint64_t)nx * multi_shard_rows(ny, band, n, r);
                        MultiTables mt = multi_tables(tr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, npix);
                        const size_t bytes = multi_place(mt, npix);
                        CHECK(bytes == multi_shard_bytes(tr, npix) && bytes == mt.bytes && bytes <= stride);
                        CHECK(mt.t[0].n == 2u + (tr.counts ? 2u : 0u) + (tr.channels ? 1u : 0u));
                        CHECK(mt.t[1].n == (tr.halves ? 4u : 0u) && mt.t[2].n == tr.buckets);
                        std::vector<std::pair<size_t, size_t>> spans; // [begin, end) of every plane in the buffer
                        size_t payload = 0;
                        for (uint32_t k = 0; k < RT_MULTI_TABLES; ++k) {
                            CHECK(mt.base[k] % 16u == 0u && mt.base[k] <= bytes);
                            for (uint32_t q = 0; q < mt.t[k].n; ++q) {
                                const Plane& pl = mt.t[k].row[q];
                                const size_t at = mt.base[k] + pl.stage, len = plane_bytes(pl, npix);
                                CHECK(at % (pl.elem_bytes % 16u == 0u ? 16u : pl.elem_bytes % 4u == 0u ? 4u : 1u) == 0u);
                                CHECK(at + len <= bytes);
                                spans.emplace_back(at, at + len), payload += len;
                            }
                        }
                        for (size_t a = 0; a < spans.size(); ++a)
                            for (size_t b = a + 1; b < spans.size(); ++b) CHECK(spans[a].second <= spans[b].first || spans[b].second <= spans[a].first);
                        const size_t per_pixel = accum_state_pixel_bytes((tr.counts ? RT_ACCUM_STATE_COUNTS : 0u) | (tr.channels ? RT_ACCUM_STATE_CHANNELS : 0u)) +
                                                 (tr.halves ? RT_HALVES_PIXEL_BYTES : 0u) + buckets_pixel_bytes(tr.buckets);
                        CHECK(payload == npix * per_pixel && bytes < payload + 16u * RT_MULTI_TABLES);
                    }
                }
    section("placement");
}

// A whole-frame snapshot whose every value is its own (plane, pixel, part) index, in arrays of exactly the header's sizes
struct Whole {
    std::vector<float> sum, hsum[2], bsum[RT_BUCKETS_MAX];
    std::vector<double> mom, chm, hmom[2];
    std::vector<uint32_t> cnt;
    std::vector<uint8_t> conv;
    RtAccumState st{};
    RtAccumHalves hs{};
    RtAccumBuckets bs{};
    // f64: the index as a number (exact); f32: the index as the bit pattern (plane < 32, pixel < 2^24, part < 4), compared as bits
    static double value(uint32_t plane, uint64_t pixel, uint32_t part) { return (double)(plane * 64u + part) * 4194304.0 + (double)pixel; }
    static uint32_t bits(uint32_t plane, uint64_t pixel, uint32_t part) { return plane << 26 | (uint32_t)pixel << 2 | part; }
    static void fill(std::vector<double>& v, uint32_t plane, uint64_t npix, uint32_t parts) {
        v.resize(npix * parts);
        for (uint64_t p = 0; p < npix; ++p)
            for (uint32_t k = 0; k < parts; ++k) v[p * parts + k] = value(plane, p, k);
    }
    static void fill(std::vector<float>& v, uint32_t plane, uint64_t npix, uint32_t parts) {
        v.resize(npix * parts);
        for (uint64_t p = 0; p < npix; ++p)
            for (uint32_t k = 0; k < parts; ++k) {
                const uint32_t b = bits(plane, p, k);
                std::memcpy(&v[p * parts + k], &b, sizeof(b));
            }
    }
    static bool is(float f, uint32_t plane, uint64_t pixel, uint32_t part) {
        uint32_t b;
        std::memcpy(&b, &f, sizeof(b));
        return b == bits(plane, pixel, part);
    }
    Whole(uint32_t nx, uint32_t ny, uint32_t planes, uint32_t M) {
        const uint64_t npix = (uint64_t)nx * ny;
        st.nx = nx, st.rows = ny, st.first_sample = 3u, st.done = 40u, st.planes = planes, st.frame_id = 77u;
        fill(sum, 1u, npix, 3u), fill(mom, 2u, npix, 2u);
        st.sum = sum.data(), st.moments = mom.data();
        if (planes & RT_ACCUM_STATE_COUNTS) {
            cnt.assign(npix, 0u), conv.assign(npix, 0u);
            for (uint64_t p = 0; p < npix; ++p) conv[p] = (uint8_t)(p % 3u == 1u), cnt[p] = conv[p] ? (uint32_t)(p % 40u) : 40u;
            st.counts = cnt.data(), st.converged = conv.data();
        }
        if (planes & RT_ACCUM_STATE_CHANNELS) fill(chm, 3u, npix, 6u), st.channel_moments = chm.data();
        hs.nx = nx, hs.rows = ny, hs.first_sample = 3u, hs.done = 40u, hs.frame_id = 77u;
        for (uint32_t h = 0; h < 2u; ++h) {
            fill(hsum[h], 4u + h, npix, 3u), fill(hmom[h], 6u + h, npix, 2u);
            hs.sum[h] = hsum[h].data(), hs.moments[h] = hmom[h].data();
        }
        bs.nx = nx, bs.rows = ny, bs.first_sample = 3u, bs.done = 40u, bs.frame_id = 77u, bs.M = M;
        for (uint32_t b = 0; b < M; ++b) fill(bsum[b], 8u + b, npix, 3u), bs.sum[b] = bsum[b].data();
    }
};

static RtCamera test_camera() {
    RtCamera cam{};
    for (int k = 0; k < 3; ++k) cam.origin[k] = 1.0f + k, cam.horizontal[k] = 0.5f * k, cam.vertical[k] = -1.0f * k, cam.lower_left_corner[k] = 0.25f;
    return cam;
}

// The host split: scalar fields, frame_id of the shard, and every element of every plane the value of the image pixel it belongs to.
static void split() {
    const RtCamera cam = test_camera();
    for (const auto& sz : SIZES)
        for (const uint32_t band : BANDS)
            for (const uint32_t n : COUNTS)
                for (const uint32_t planes : {0u, (uint32_t)RT_ACCUM_STATE_COUNTS, (uint32_t)(RT_ACCUM_STATE_COUNTS | RT_ACCUM_STATE_CHANNELS)}) {
                    const uint32_t nx = sz[0], ny = sz[1];
                    if ((uint64_t)nx * ny > 100000u && (planes != (RT_ACCUM_STATE_COUNTS | RT_ACCUM_STATE_CHANNELS) || band != 8u || n < 3u)) continue; // (the large frame: every plane, n = 3 and 8)
                    const uint32_t M = planes ? 16u : 3u;
                    const Whole w(nx, ny, planes, M);
                    RtParams prm{};
                    prm.nx = nx, prm.ny = ny, prm.spp = 4u, prm.max_depth = 50, prm.seed = 9u, prm.shard_band = band, prm.shard_count = 1u;
                    CHECK(accum_state_invalid(&w.st) == nullptr);
                    for (uint32_t r = 0; r < n; ++r) {
                        const bool tracked = planes != RT_ACCUM_STATE_COUNTS; // once without halves and buckets
                        ShardSnapshot s;
                        multi_split(cam, prm, n, r, w.st, tracked ? &w.hs : nullptr, tracked ? &w.bs : nullptr, s);
                        const uint32_t rows = multi_shard_rows(ny, band, n, r);
                        const RtParams sp = multi_shard_params(prm, n, r);
                        CHECK(sp.shard_band == band && sp.shard_count == n && sp.shard_id == r);
                        CHECK(s.st.nx == nx && s.st.rows == rows && s.st.first_sample == 3u && s.st.done == 40u && s.st.planes == planes && s.st.reserved == 0u);
                        CHECK(s.st.frame_id == accum_frame_id(cam, sp));
                        CHECK(n > 1u || s.st.frame_id == accum_frame_id(cam, prm));
                        CHECK(accum_state_invalid(&s.st) == nullptr); // (reads counts and converged over all rows * nx: a short array is a report)
                        CHECK(((planes & RT_ACCUM_STATE_COUNTS) != 0u) == (s.st.counts != nullptr) && ((planes & RT_ACCUM_STATE_CHANNELS) != 0u) == (s.st.channel_moments != nullptr));
                        if (tracked) {
                            CHECK(accum_halves_invalid(&s.hs) == nullptr && accum_buckets_invalid(&s.bs) == nullptr);
                            CHECK(s.hs.nx == nx && s.hs.rows == rows && s.hs.first_sample == 3u && s.hs.done == 40u && s.hs.frame_id == s.st.frame_id);
                            CHECK(s.bs.nx == nx && s.bs.rows == rows && s.bs.first_sample == 3u && s.bs.done == 40u && s.bs.frame_id == s.st.frame_id && s.bs.M == M);
                        }
                        bool same = true;
                        for (uint32_t lj = 0; lj < rows; ++lj)
                            for (uint32_t i = 0; i < nx; ++i) {
                                const uint64_t lp = (uint64_t)lj * nx + i, p = (uint64_t)multi_image_row(lj, band, n, r) * nx + i;
                                for (uint32_t k = 0; k < 3u; ++k) same = same && Whole::is(s.st.sum[lp * 3 + k], 1u, p, k);
                                for (uint32_t k = 0; k < 2u; ++k) same = same && s.st.moments[lp * 2 + k] == Whole::value(2u, p, k);
                                if (planes & RT_ACCUM_STATE_COUNTS) same = same && s.st.counts[lp] == w.cnt[p] && s.st.converged[lp] == w.conv[p];
                                if (planes & RT_ACCUM_STATE_CHANNELS)
                                    for (uint32_t k = 0; k < 6u; ++k) same = same && s.st.channel_moments[lp * 6 + k] == Whole::value(3u, p, k);
                                if (!tracked) continue;
                                for (uint32_t h = 0; h < 2u; ++h) {
                                    for (uint32_t k = 0; k < 3u; ++k) same = same && Whole::is(s.hs.sum[h][lp * 3 + k], 4u + h, p, k);
                                    for (uint32_t k = 0; k < 2u; ++k) same = same && s.hs.moments[h][lp * 2 + k] == Whole::value(6u + h, p, k);
                                }
                                for (uint32_t b = 0; b < M; ++b)
                                    for (uint32_t k = 0; k < 3u; ++k) same = same && Whole::is(s.bs.sum[b][lp * 3 + k], 8u + b, p, k);
                            }
                        CHECK(same);
                    }
                }
    section("split");
}

// A shard without rows: a well-formed snapshot of no pixels whose pointers are not NULL.
static void empty_shard() {
    const RtCamera cam = test_camera();
    const Whole w(16u, 11u, RT_ACCUM_STATE_COUNTS | RT_ACCUM_STATE_CHANNELS, 3u);
    RtParams prm{};
    prm.nx = 16u, prm.ny = 11u, prm.spp = 1u, prm.max_depth = 5, prm.shard_band = 0u; // 0 = 8: two bands for three shards
    CHECK(multi_shard_rows(11u, 8u, 3u, 2u) == 0u);
    ShardSnapshot s;
    multi_split(cam, prm, 3u, 2u, w.st, &w.hs, &w.bs, s);
    CHECK(s.st.rows == 0u && s.st.nx == 16u && s.hs.rows == 0u && s.bs.rows == 0u);
    CHECK(accum_state_invalid(&s.st) == nullptr && accum_halves_invalid(&s.hs) == nullptr && accum_buckets_invalid(&s.bs) == nullptr);
    CHECK(s.st.sum && s.st.moments && s.st.counts && s.st.converged && s.st.channel_moments);
    const MultiTracked all{true, true, true, 3u};
    CHECK(multi_shard_bytes(all, 0u) == 0u);
    CHECK(multi_slot_stride(all, 16u, multi_rows_pad(11u, 8u, 3u)) >= multi_shard_bytes(all, 16u * 8u));
    // the one-pixel frame on two devices: the second shard is empty
    const Whole one(1u, 1u, 0u, 3u);
    prm.nx = prm.ny = 1u;
    ShardSnapshot a, b;
    multi_split(cam, prm, 2u, 0u, one.st, nullptr, nullptr, a);
    multi_split(cam, prm, 2u, 1u, one.st, nullptr, nullptr, b);
    CHECK(a.st.rows == 1u && b.st.rows == 0u && a.st.sum[2] == one.sum[2] && a.st.moments[1] == one.mom[1]);
    CHECK(a.st.frame_id != b.st.frame_id && accum_state_invalid(&b.st) == nullptr && !b.hs.sum[0] && !b.bs.sum[0]);
    section("empty_shard");
}

int main() {
    row_map();
    placement();
    split();
    empty_shard();
    std::printf("ok\n");
    return 0;
}
