// The GPU-free arithmetic of adaptive sampling (csrc/rt_adaptive_plan.h) as a stand-alone program: built with AddressSanitizer + UBSan by
// tests/test_adaptive_host.py and run without a GPU.  It prints one line per section — its name and the number of checks made — and "ok";
// a failed check prints what failed and ends the program with status 1.
#include "rt_adaptive_plan.h"

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
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- the ranges of RtAdaptive
    const RtAdaptive good{0.05, 0.01, 2u, 0u};
    CHECK(adaptive_invalid(&good, 1u) == nullptr);
    CHECK(adaptive_invalid(nullptr, 1u) != nullptr);
    CHECK(adaptive_invalid(&good, 0u) != nullptr);
    for (double t : {-1.0, -0.0 - 1e-300, inf, -inf, nan}) {
        RtAdaptive a = good;
        a.tolerance = t;
        CHECK(adaptive_invalid(&a, 1u) != nullptr);
    }
    for (double t : {0.0, 1e-300, 1e300}) {
        RtAdaptive a = good;
        a.tolerance = t;
        CHECK(adaptive_invalid(&a, 1u) == nullptr);
    }
    for (double f : {0.0, -1.0, inf, nan}) {
        RtAdaptive a = good;
        a.luminance_floor = f;
        CHECK(adaptive_invalid(&a, 1u) != nullptr);
    }
    for (uint32_t m : {0u, 1u}) {
        RtAdaptive a = good;
        a.min_samples = m;
        CHECK(adaptive_invalid(&a, 1u) != nullptr);
    }
    {
        RtAdaptive a = good;
        a.reserved = 1u;
        CHECK(adaptive_invalid(&a, 1u) != nullptr);
        a.reserved = 0u, a.min_samples = 0xFFFFFFFFu;
        CHECK(adaptive_invalid(&a, 0xFFFFFFFFu) == nullptr);
    }
    section("ranges");
    // ---- the figures of a pixel: constant samples have no variance, n < 2 has none by definition
    for (uint32_t n = 0; n <= 64u; ++n)
        for (double y : {0.0, 0.25, 1.0, 3.0}) {
            double ybar, v;
            adaptive_pixel_figures(y * n, y * y * n, n, ybar, v);
            CHECK(v == 0.0);
            CHECK(ybar == (n ? y : 0.0));
        }
    section("figures");
    // ---- the criterion on both sides of equality: S1 = 8, S2 = 19, n = 4: Ybar = 2, V = ((19 - 16) / 3) / 4 = 0.25 exactly
    {
        double ybar, v;
        adaptive_pixel_figures(8.0, 19.0, 4u, ybar, v);
        CHECK(ybar == 2.0 && v == 0.25);
        RtAdaptive a{0.25, 0.5, 4u, 0u}; // thr = 0.25 * 2 = 0.5, thr^2 = 0.25 = V
        CHECK(adaptive_converged_moments(8.0, 19.0, 4u, a));
        a.tolerance = std::nextafter(0.25, 0.0);
        CHECK(!adaptive_converged_moments(8.0, 19.0, 4u, a));
        a.tolerance = 0.25, a.min_samples = 5u;
        CHECK(!adaptive_converged_moments(8.0, 19.0, 4u, a)); // n < min_samples
        a.min_samples = 4u, a.luminance_floor = 4.0;           // the floor above Ybar: thr = 0.25 * 4
        a.tolerance = 0.125;
        CHECK(adaptive_converged_moments(8.0, 19.0, 4u, a));
        a.tolerance = std::nextafter(0.125, 0.0);
        CHECK(!adaptive_converged_moments(8.0, 19.0, 4u, a));
        // no variance: converged for every tolerance, 0 included, from min_samples on
        a = RtAdaptive{0.0, 0.01, 2u, 0u};
        CHECK(adaptive_converged_moments(0.0, 0.0, 2u, a) && !adaptive_converged_moments(0.0, 0.0, 1u, a));
        CHECK(!adaptive_converged_moments(8.0, 19.0, 4u, a));
        // a non-finite sample never converges, whatever the tolerance
        a = RtAdaptive{1e300, 0.01, 2u, 0u};
        // (the moments a non-finite luminance Y leaves: S1 += Y, S2 += Y * Y)
        CHECK(!adaptive_converged_moments(nan, nan, 8u, a));
        CHECK(!adaptive_converged_moments(inf, inf, 8u, a));
        CHECK(!adaptive_converged_moments(-inf, inf, 8u, a));
        CHECK(!adaptive_converged_moments(nan, 1.0, 8u, a));
        CHECK(!adaptive_converged_moments(1.0, nan, 8u, a));
        CHECK(adaptive_converged_moments(8.0, 19.0, 4u, a));
    }
    // a negative variance estimate (cancellation) clamps to 0 and converges
    {
        const RtAdaptive a{0.0, 0.01, 2u, 0u};
        CHECK(adaptive_converged_moments(3.0, 2.9999999, 3u, a));
    }
    section("criterion");
    // ---- monotone in the tolerance: once converged, converged for every larger tolerance
    {
        std::vector<double> tol;
        for (int e = -40; e <= 40; ++e) tol.push_back(std::ldexp(1.0, e));
        uint64_t state = 0x9E3779B97F4A7C15ull;
        auto next = [&]() {
            state ^= state << 13, state ^= state >> 7, state ^= state << 17;
            return (double)(state >> 11) / 9007199254740992.0;
        };
        for (int trial = 0; trial < 2000; ++trial) {
            const uint32_t n = 2u + (uint32_t)(next() * 60.0);
            double s1 = 0.0, s2 = 0.0;
            for (uint32_t k = 0; k < n; ++k) {
                const double y = next() * next() * 4.0;
                s1 += y, s2 += y * y;
            }
            bool seen = false;
            for (double t : tol) {
                const RtAdaptive a{t, 0.01, 2u, 0u};
                const bool c = adaptive_converged_moments(s1, s2, n, a);
                CHECK(c || !seen);
                seen = seen || c;
            }
            CHECK(seen);
        }
    }
    section("monotone");
    std::printf("ok\n");
    return 0;
}
