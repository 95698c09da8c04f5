// The GPU-free arithmetic of the display transform (csrc/rt_display_plan.h) as a stand-alone program: built with AddressSanitizer + UBSan
// by tests/test_display_host.py and run without a GPU.  It prints one line per section — its name and the number of checks made — and
// "ok"; a failed check prints what failed and ends the program with status 1.
#include "rt_display_plan.h"

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
static uint32_t bits_of(float f) {
    uint32_t b;
    std::memcpy(&b, &f, sizeof(b));
    return b;
}

int main() {
    using namespace rt;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- rt_display_check: every refusal, and what is ignored where it does not apply
    const RtDisplay good{RT_EXPOSURE_PERCENTILE, 0.5f, 0.99f, RT_TONE_REINHARD, 4.0f, RT_TRANSFER_SRGB, RT_DITHER_BAYER8, 0u};
    CHECK(display_invalid(&good) == nullptr);
    CHECK(display_invalid(nullptr) != nullptr);
    {
        RtDisplay b = good;
        b.exposure_mode = 3u;
        CHECK(display_invalid(&b) != nullptr);
        b = good, b.curve = 3u;
        CHECK(display_invalid(&b) != nullptr);
        b = good, b.transfer = 2u;
        CHECK(display_invalid(&b) != nullptr);
        b = good, b.dither = 2u;
        CHECK(display_invalid(&b) != nullptr);
        b = good, b.reserved = 1u;
        CHECK(display_invalid(&b) != nullptr);
        for (float v : {0.0f, -1.0f, inf, -inf, nan}) {
            b = good, b.exposure_value = v;
            CHECK(display_invalid(&b) != nullptr);
        }
        b = good, b.exposure_value = 1e-45f; // (the smallest denormal is finite and > 0)
        CHECK(display_invalid(&b) == nullptr);
        for (float q : {0.0f, -0.5f, 1.0000001f, inf, nan}) {
            b = good, b.percentile = q;
            CHECK(display_invalid(&b) != nullptr);
            b.exposure_mode = RT_EXPOSURE_KEY; // ignored
            CHECK(display_invalid(&b) == nullptr);
        }
        b = good, b.percentile = 1.0f;
        CHECK(display_invalid(&b) == nullptr);
        for (float w : {0.0f, -1.0f, -inf, nan}) {
            b = good, b.white = w;
            CHECK(display_invalid(&b) != nullptr);
            b.curve = RT_TONE_ACES; // ignored
            CHECK(display_invalid(&b) == nullptr);
        }
        b = good, b.white = inf;
        CHECK(display_invalid(&b) == nullptr);
    }
    section("check");

    // ---- B: the permutation, its first row, and the recursive definition of the Bayer matrix
    {
        const uint32_t first[8] = {0u, 32u, 8u, 40u, 2u, 34u, 10u, 42u};
        std::vector<int> seen(64, 0);
        for (uint32_t y = 0; y < 8; ++y)
            for (uint32_t x = 0; x < 8; ++x) {
                const uint32_t b = display_bayer(x, y);
                CHECK(b < 64u);
                ++seen[b];
                if (y == 0u) CHECK(b == first[x]);
            }
        for (int k = 0; k < 64; ++k) CHECK(seen[k] == 1);
        const uint32_t m2[2][2] = {{0u, 2u}, {3u, 1u}}; // M_2n = [[4 M, 4 M + 2], [4 M + 3, 4 M + 1]]
        for (uint32_t y = 0; y < 8; ++y)
            for (uint32_t x = 0; x < 8; ++x)
                CHECK(display_bayer(x, y) == 16u * m2[y & 1u][x & 1u] + 4u * m2[(y >> 1) & 1u][(x >> 1) & 1u] + m2[(y >> 2) & 1u][(x >> 2) & 1u]);
    }
    section("bayer");

    // ---- the rank: max(1, ceil(q n)), never above n
    CHECK(display_rank(1.0f, 1u) == 1u && display_rank(1.0f, 66000u) == 66000u && display_rank(1.0f, (1ull << 28)) == (1ull << 28));
    CHECK(display_rank(9.5367431640625e-07f, 1u) == 1u && display_rank(9.5367431640625e-07f, 66000u) == 1u);
    CHECK(display_rank(9.5367431640625e-07f, (1u << 20) + 1u) == 2u && display_rank(9.5367431640625e-07f, 1u << 20) == 1u);
    CHECK(display_rank(0.5f, 1u) == 1u && display_rank(0.5f, 2u) == 1u && display_rank(0.5f, 3u) == 2u && display_rank(0.5f, 66000u) == 33000u);
    CHECK(display_rank(0.99f, 100u) == 100u); // (0.99f is a little above 0.99: 99.0000002 rounds up)
    CHECK(display_rank(0.75f, 100u) == 75u);
    for (uint64_t n : {1ull, 2ull, 255ull, 66000ull, 8294400ull, 1ull << 28})
        for (float q : {9.5367431640625e-07f, 0.01f, 0.5f, 0.99f, 1.0f}) {
            const uint64_t r = display_rank(q, n);
            CHECK(r >= 1u && r <= n);
            CHECK((double)r >= (double)q * (double)n && ((double)r - 1.0 < (double)q * (double)n || r == 1u));
        }
    section("rank");

    // ---- the bin search, the bins' edges and midpoints
    {
        std::vector<uint32_t> h(RT_DISPLAY_BINS, 0u);
        CHECK(display_bin_search(h.data(), 1u) == RT_DISPLAY_BINS); // nothing lit
        h[0] = 7u;                                                  // all mass in bin 0 (denormals and the first eighth of FLT_MIN's octave)
        CHECK(display_bin_search(h.data(), 1u) == 0u && display_bin_search(h.data(), 7u) == 0u && display_bin_search(h.data(), 8u) == RT_DISPLAY_BINS);
        h[0] = 0u, h[RT_DISPLAY_LAST_BIN] = 5u; // all mass in bin 2039
        CHECK(display_bin_search(h.data(), 1u) == RT_DISPLAY_LAST_BIN && display_bin_search(h.data(), 5u) == RT_DISPLAY_LAST_BIN);
        h[RT_DISPLAY_LAST_BIN] = 0u, h[1000] = 1u; // n_lit = 1
        CHECK(display_bin_search(h.data(), display_rank(1.0f, 1u)) == 1000u && display_bin_search(h.data(), display_rank(1e-6f, 1u)) == 1000u);
        h[1000] = 3u, h[1016] = 4u, h[1100] = 0xFFFFFFFFu; // the cumulative count passes 2^32
        CHECK(display_bin_search(h.data(), 3u) == 1000u && display_bin_search(h.data(), 4u) == 1016u && display_bin_search(h.data(), 7u) == 1016u);
        CHECK(display_bin_search(h.data(), 8u) == 1100u && display_bin_search(h.data(), 7ull + 0xFFFFFFFFull) == 1100u);
        CHECK(display_bin_search(h.data(), 8ull + 0xFFFFFFFFull) == RT_DISPLAY_BINS);
        CHECK(display_bin_of_bits(0x00000001u) == 0u && display_bin_of_bits(bits_of(1.17549435e-38f)) == 8u);
        CHECK(display_bin_of_bits(0x3F7FFFFFu) == 1015u && display_bin_of_bits(bits_of(1.0f)) == 1016u);
        CHECK(display_bin_of_bits(bits_of(3.402823466e+38f)) == RT_DISPLAY_LAST_BIN && display_bin_of_bits(bits_of(inf)) == RT_DISPLAY_LAST_BIN + 1u);
        CHECK(display_bin_mid(1016u) == 1.0625f && display_bin_mid(1015u) == 0.96875f && display_bin_mid(1023u) == 1.9375f);
        for (uint32_t b = 0; b <= RT_DISPLAY_LAST_BIN; ++b) {
            CHECK(display_bin_of_bits(display_bin_mid_bits(b)) == b && std::isfinite(display_bin_mid(b)) && display_bin_mid(b) > 0.0f);
            if (b) CHECK(display_bin_mid(b) > display_bin_mid(b - 1u));
        }
    }
    section("bins");

    // ---- e: the quotient rounded to f32, and 1 where it is zero or not finite
    CHECK(display_exposure(0.18f, 0.5) == (float)((double)0.18f / 0.5) && display_exposure(1.0f, (double)1.0625f) == (float)(1.0 / 1.0625));
    CHECK(display_exposure(1.0f, 0.0) == 1.0f && display_exposure(1.0f, (double)inf) == 1.0f && display_exposure(1.0f, (double)nan) == 1.0f);
    CHECK(display_exposure(1e30f, 1e-30) == 1.0f && display_exposure(1e-30f, 1e30) == 1.0f); // the quotient rounds to inf, to 0
    CHECK(display_exposure(1e-30f, 1e10) == (float)((double)1e-30f / 1e10));                 // a denormal e stays
    section("exposure");
    std::printf("ok\n");
    return 0;
}
