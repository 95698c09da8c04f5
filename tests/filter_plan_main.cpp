// The GPU-free arithmetic of the pixel filters (csrc/rt_filter_plan.h, and the filter's row in csrc/rt_accum_planes.h) as a stand-alone
// program: built with AddressSanitizer + UBSan by tests/test_filter_host.py and run without a GPU.  It prints one line per section — its
// name and the number of checks made — and "ok"; a failed check prints what failed and ends the program with status 1.
#include "rt_accum_planes.h"
#include "rt_filter_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

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

int main() {
    using namespace rt;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const RtPixelFilter defaults[5] = {{RT_FILTER_BOX, 0.5f, 0.0f, 0.0f},
                                       {RT_FILTER_TENT, 1.0f, 0.0f, 0.0f},
                                       {RT_FILTER_GAUSSIAN, 1.5f, 0.5f, 0.0f},
                                       {RT_FILTER_MITCHELL, 2.0f, 1.0f / 3.0f, 1.0f / 3.0f},
                                       {RT_FILTER_BLACKMAN_HARRIS, 1.5f, 0.0f, 0.0f}};
    // ---- rt_pixel_filter_check: each refusal
    CHECK(pixel_filter_invalid(nullptr) != nullptr);
    for (const RtPixelFilter& good : defaults) {
        CHECK(pixel_filter_invalid(&good) == nullptr);
        RtPixelFilter b = good;
        b.kind = RT_FILTER_BLACKMAN_HARRIS + 1u;
        CHECK(pixel_filter_invalid(&b) != nullptr);
        for (const float bad : {nan, inf, -inf}) {
            b = good, b.radius = bad;
            CHECK(pixel_filter_invalid(&b) != nullptr);
            b = good, b.p0 = bad;
            CHECK(pixel_filter_invalid(&b) != nullptr);
            b = good, b.p1 = bad;
            CHECK(pixel_filter_invalid(&b) != nullptr);
        }
        for (const float r : {0.0f, -1.0f, std::nextafter(0.5f, 0.0f), std::nextafter(3.0f, 4.0f), 100.0f}) {
            b = good, b.radius = r;
            CHECK(pixel_filter_invalid(&b) != nullptr);
        }
        for (const float r : {0.5f, 3.0f, 1.25f}) {
            b = good, b.radius = r;
            CHECK(pixel_filter_invalid(&b) == nullptr);
        }
    }
    for (const float s : {0.0f, -0.5f}) {
        RtPixelFilter b = defaults[2];
        b.p0 = s;
        CHECK(pixel_filter_invalid(&b) != nullptr);
        b = defaults[1], b.p0 = s; // (sigma is the Gaussian's alone)
        CHECK(pixel_filter_invalid(&b) == nullptr);
    }
    section("check");

    // ---- the table: every entry finite, the value at the centre the largest, box all ones, NULL outputs, a refused filter writes nothing
    for (const RtPixelFilter& f : defaults) {
        std::vector<float> table(RT_FILTER_TABLE, nan); // exactly RT_FILTER_TABLE entries: one past them is a heap overflow
        uint32_t reach = 99u;
        CHECK(pixel_filter_table(&f, table.data(), &reach) == nullptr);
        for (uint32_t k = 0; k < RT_FILTER_TABLE; ++k) CHECK(std::isfinite(table[k]) && table[k] <= table[0]);
        CHECK(table[0] > 0.88f && table[0] <= 1.0f);
        if (f.kind == RT_FILTER_BOX)
            for (uint32_t k = 0; k < RT_FILTER_TABLE; ++k) CHECK(table[k] == 1.0f);
        if (f.kind == RT_FILTER_TENT) CHECK(table[0] == 1.0f - 0.5f / 256.0f && table[255] == 0.5f / 256.0f);
        if (f.kind == RT_FILTER_MITCHELL) CHECK(table[255] < 0.0f && table[200] < 0.0f); // the negative lobe
        CHECK(reach == pixel_filter_reach(f.radius));
        CHECK(pixel_filter_table(&f, nullptr, nullptr) == nullptr);
        CHECK(pixel_filter_table(&f, nullptr, &reach) == nullptr && pixel_filter_table(&f, table.data(), nullptr) == nullptr);
        RtPixelFilter b = f;
        b.radius = 4.0f;
        float one = 7.0f;
        reach = 99u;
        CHECK(pixel_filter_table(&b, &one, &reach) != nullptr && one == 7.0f && reach == 99u);
    }
    CHECK(pixel_filter_table(nullptr, nullptr, nullptr) != nullptr);
    section("table");

    // ---- the reach and the index scale
    CHECK(pixel_filter_reach(0.5f) == 0u && pixel_filter_reach(std::nextafter(0.5f, 1.0f)) == 1u && pixel_filter_reach(1.0f) == 1u);
    CHECK(pixel_filter_reach(1.5f) == 1u && pixel_filter_reach(std::nextafter(1.5f, 2.0f)) == 2u && pixel_filter_reach(2.0f) == 2u);
    CHECK(pixel_filter_reach(2.5f) == 2u && pixel_filter_reach(std::nextafter(2.5f, 3.0f)) == 3u && pixel_filter_reach(3.0f) == 3u);
    for (const float r : {0.5f, 0.75f, 1.0f, 1.5f, 2.0f, 2.9f, 3.0f}) {
        const float scale = pixel_filter_scale(r);
        CHECK(scale == 256.0f / r);
        CHECK((uint32_t)(r * scale) >= 255u && (uint32_t)(r * scale) <= 257u); // the edge of the support lands on the last entry once clamped
    }
    section("reach");

    // ---- rt_accum_filter_check: each refusal, and that the plane is not read (it is one element long)
    std::vector<float> plane(4);
    RtAccumFilter good{};
    good.nx = 1000u, good.rows = 1000u, good.first_sample = 3u, good.done = 7u, good.frame_id = 42u;
    good.filter = defaults[3], good.plane = plane.data();
    CHECK(accum_filter_invalid(&good) == nullptr);
    CHECK(accum_filter_invalid(nullptr) != nullptr);
    for (int k = 0; k < 2; ++k) {
        RtAccumFilter b = good;
        b.reserved[k] = 1u;
        CHECK(accum_filter_invalid(&b) != nullptr);
    }
    {
        RtAccumFilter b = good;
        b.plane = nullptr;
        CHECK(accum_filter_invalid(&b) != nullptr);
        b = good, b.filter.radius = 0.25f;
        CHECK(accum_filter_invalid(&b) != nullptr);
        b = good, b.filter.kind = 5u;
        CHECK(accum_filter_invalid(&b) != nullptr);
        b = good, b.first_sample = 0xFFFFFFFFu - 7u;
        CHECK(accum_filter_invalid(&b) == nullptr);
        b.first_sample += 1u;
        CHECK(accum_filter_invalid(&b) != nullptr);
        b = good, b.nx = 0u, b.rows = 0u, b.done = 0u;
        CHECK(accum_filter_invalid(&b) == nullptr);
    }
    CHECK(pixel_filter_same(defaults[3], defaults[3]) && !pixel_filter_same(defaults[3], defaults[2]));
    {
        RtPixelFilter z = defaults[1], mz = defaults[1];
        mz.p1 = -0.0f;
        CHECK(!pixel_filter_same(z, mz)); // by bits
    }
    section("snapshot");

    // ---- the plane as a table row: one 16 B row, staged at 0, sized by the pixels; the buffer holds the table in front of it
    for (uint64_t npix : {0ull, 1ull, 255ull, 257ull, 1920ull * 1080ull}) {
        char local[1];
        PlaneTable t = filter_planes(good, local);
        CHECK(t.n == 1u && t.row[0].elem_bytes == 16u && t.row[0].parts == 1u && t.row[0].host == plane.data() && t.row[0].local == local);
        CHECK(planes_place(t, npix) == npix * RT_FILTER_PIXEL_BYTES && t.row[0].stage == 0u && RT_FILTER_PIXEL_BYTES == 16u);
        CHECK(filter_buffer_bytes(npix) == 1024u + npix * 16u && RT_FILTER_TABLE_BYTES % 16u == 0u);
    }
    {
        SnapshotHeader h = snapshot_header(good);
        CHECK(h.nx == 1000u && h.rows == 1000u && h.first_sample == 3u && h.done == 7u && h.frame_id == 42u);
        CHECK(snapshot_mismatch(h, h, "filter plane", SNAPSHOT_FIRST_AND_DONE).empty());
        SnapshotHeader o = h;
        o.done = 8u;
        CHECK(!snapshot_mismatch(h, o, "filter plane", SNAPSHOT_FIRST_AND_DONE).empty());
    }
    section("planes");
    std::printf("ok\n");
    return 0;
}
