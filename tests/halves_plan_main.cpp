// The GPU-free arithmetic of the half buffers (csrc/rt_halves_plan.h) as a stand-alone program: built with AddressSanitizer + UBSan by
// tests/test_halves_host.py and run without a GPU.  It prints one line per section — its name and the number of checks made — and "ok";
// a failed check prints what failed and ends the program with status 1.
#include "rt_halves_plan.h"

#include <cstdio>
#include <cstdlib>
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
    // ---- n_h against brute force over the absolute indices (64-bit, so that the window may end at 2^32 - 1)
    for (uint64_t first : {0ull, 1ull, 0xFFFFFFFEull})
        for (uint64_t n = 0; n <= 9 && first + n <= 0xFFFFFFFFull; ++n) {
            uint32_t brute[2] = {0u, 0u};
            for (uint64_t i = first; i < first + n; ++i) ++brute[i & 1u];
            for (uint32_t h = 0; h < 2; ++h) CHECK(halves_count((uint32_t)first, (uint32_t)n, h) == brute[h]);
            CHECK(halves_count((uint32_t)first, (uint32_t)n, 0u) + halves_count((uint32_t)first, (uint32_t)n, 1u) == n);
        }
    CHECK(halves_count(0u, 0xFFFFFFFFu, 0u) == 0x80000000u && halves_count(0u, 0xFFFFFFFFu, 1u) == 0x7FFFFFFFu);
    CHECK(halves_count(1u, 0xFFFFFFFEu, 0u) == 0x7FFFFFFFu && halves_count(1u, 0xFFFFFFFEu, 1u) == 0x7FFFFFFFu);
    CHECK(halves_count(0xFFFFFFFFu, 0xFFFFFFFFu, 0u) == 0x7FFFFFFFu); // (no such window exists; the count still forms no sum that wraps)
    section("counts");

    // ---- rt_accum_halves_check: each refusal, and that no plane is read (the planes are one element long)
    std::vector<float> s0(3), s1(3);
    std::vector<double> m0(2), m1(2);
    RtAccumHalves good{};
    good.nx = 1000u, good.rows = 1000u, good.first_sample = 3u, good.done = 7u, good.frame_id = 42u;
    good.sum[0] = s0.data(), good.sum[1] = s1.data(), good.moments[0] = m0.data(), good.moments[1] = m1.data();
    CHECK(accum_halves_invalid(&good) == nullptr);
    CHECK(accum_halves_invalid(nullptr) != nullptr);
    for (int k = 0; k < 2; ++k) {
        RtAccumHalves b = good;
        b.reserved[k] = 1u;
        CHECK(accum_halves_invalid(&b) != nullptr);
        b = good, b.sum[k] = nullptr;
        CHECK(accum_halves_invalid(&b) != nullptr);
        b = good, b.moments[k] = nullptr;
        CHECK(accum_halves_invalid(&b) != nullptr);
    }
    {
        RtAccumHalves b = good;
        b.first_sample = 0xFFFFFFFFu - 7u;
        CHECK(accum_halves_invalid(&b) == nullptr);
        b.first_sample += 1u;
        CHECK(accum_halves_invalid(&b) != nullptr);
        b = good, b.nx = 0u, b.rows = 0u, b.done = 0u;
        CHECK(accum_halves_invalid(&b) == nullptr);
    }
    section("check");

    // ---- the layout: four planes, disjoint, aligned, 56 B per pixel
    for (uint64_t npix : {0ull, 1ull, 255ull, 257ull, 1920ull * 1080ull}) {
        const HalvesLayout l = halves_layout(npix);
        CHECK(l.total == npix * RT_HALVES_PIXEL_BYTES && RT_HALVES_PIXEL_BYTES == 56u);
        CHECK(l.moments[0] == 0u && l.moments[1] == npix * 16u && l.sum[0] == npix * 32u && l.sum[1] == npix * 44u);
        CHECK(l.moments[1] % 16u == 0u && l.sum[0] % 4u == 0u && l.sum[1] % 4u == 0u);
    }
    section("layout");
    std::printf("ok\n");
    return 0;
}
