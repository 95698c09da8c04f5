// The GPU-free arithmetic of the glare (csrc/rt_glare_plan.h) as a stand-alone program: built with AddressSanitizer + UBSan by
// tests/test_glare_host.py and run without a GPU.  It prints one line per section — its name and the number of checks made — and "ok"; a
// failed check prints what failed and ends the program with status 1.
#include "rt_glare_plan.h"

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
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- rt_glare_check: every refusal, and the ends of every range
    const RtGlare good{0.1f, 0.7f, 0.0f, 6u};
    CHECK(glare_invalid(&good) == nullptr);
    CHECK(glare_invalid(nullptr) != nullptr);
    {
        RtGlare b = good;
        for (float v : {-1e-6f, 1.0000001f, inf, -inf, nan, 2.0f}) {
            b = good, b.amount = v;
            CHECK(glare_invalid(&b) != nullptr);
        }
        for (float v : {0.0f, 1.0f, 1e-45f}) {
            b = good, b.amount = v;
            CHECK(glare_invalid(&b) == nullptr);
        }
        for (float v : {0.0f, -0.5f, 1.0000001f, inf, -inf, nan}) {
            b = good, b.spread = v;
            CHECK(glare_invalid(&b) != nullptr);
        }
        for (float v : {1.0f, 1e-45f, 0.5f}) {
            b = good, b.spread = v;
            CHECK(glare_invalid(&b) == nullptr);
        }
        for (float v : {-1e-45f, -1.0f, inf, -inf, nan}) {
            b = good, b.threshold = v;
            CHECK(glare_invalid(&b) != nullptr);
        }
        for (float v : {0.0f, -0.0f, 1.0f, 3.4028234663852886e38f}) {
            b = good, b.threshold = v;
            CHECK(glare_invalid(&b) == nullptr);
        }
        for (uint32_t v : {0u, RT_GLARE_MAX_LEVELS + 1u, 0xFFFFFFFFu}) {
            b = good, b.levels = v;
            CHECK(glare_invalid(&b) != nullptr);
        }
        for (uint32_t v = 1u; v <= RT_GLARE_MAX_LEVELS; ++v) {
            b = good, b.levels = v;
            CHECK(glare_invalid(&b) == nullptr);
        }
    }
    section("check");

    // ---- Le and the level sizes
    CHECK(glare_levels(1u, 1u, 8u) == 0u && glare_levels(2u, 2u, 8u) == 1u && glare_levels(2u, 1u, 8u) == 1u && glare_levels(1u, 9u, 8u) == 4u);
    CHECK(glare_levels(5u, 1u, 8u) == 3u && glare_levels(7u, 13u, 8u) == 4u && glare_levels(7u, 13u, 3u) == 3u && glare_levels(64u, 64u, 8u) == 6u);
    CHECK(glare_levels(257u, 129u, 8u) == 8u && glare_levels(3840u, 2160u, 6u) == 6u && glare_levels(3840u, 2160u, 1u) == 1u);
    CHECK(glare_levels(0xFFFFFFFFu, 1u, 8u) == 8u && glare_levels(1u << 28, 1u, 8u) == 8u);
    {
        const RtGlare g{0.25f, 0.5f, 0.0f, 8u};
        const GlarePlan pl = glare_plan(257u, 129u, g);
        CHECK(pl.levels == 8u && pl.lv[0].nx == 257u && pl.lv[0].rows == 129u && pl.lv[8].nx == 2u && pl.lv[8].rows == 1u);
        for (uint32_t l = 1u; l <= pl.levels; ++l) {
            CHECK(pl.lv[l].nx == multiscale_half(pl.lv[l - 1u].nx) && pl.lv[l].rows == multiscale_half(pl.lv[l - 1u].rows));
            CHECK(pl.lv[l].nx % 2u == 1u || l == 8u); // odd at every level
        }
        CHECK(multiscale_half(1u) == 1u && multiscale_half(0xFFFFFFFFu) == 0x80000000u);
        const GlarePlan one = glare_plan(1u, 1u, g);
        CHECK(one.levels == 0u && one.lv[0].nx == 1u && one.lv[0].rows == 1u && one.total >= RT_GLARE_RGB_BYTES);
    }
    section("levels");

    // ---- the weights: positive, in the ratio spread, summing to 1 within Le ulp
    for (float spread : {1.0f, 0.7f, 0.5f, 0.1f, 1e-3f, 1e-30f})
        for (uint32_t le = 1u; le <= RT_GLARE_MAX_LEVELS; ++le) {
            float w[RT_GLARE_MAX_LEVELS];
            glare_weights(spread, le, w);
            double sum = 0.0;
            for (uint32_t l = 0; l < le; ++l) {
                CHECK(w[l] >= 0.0f && w[l] <= 1.0f && std::isfinite(w[l]));
                if (l) CHECK(w[l] <= w[l - 1u]);
                sum += (double)w[l];
            }
            CHECK(std::fabs(sum - 1.0) <= (double)le * 5.9604644775390625e-08);
            if (le == 1u) CHECK(w[0] == 1.0f);
            if (spread == 1.0f) CHECK(w[0] == 1.0f / (float)le && w[le - 1u] == w[0]);
        }
    section("weights");

    // ---- the scratch layout: aligned regions that neither overlap nor leave the total, for the frames of the tests and two large ones
    {
        const uint32_t frames[][2] = {{1u, 1u}, {1u, 9u}, {5u, 1u}, {2u, 2u}, {7u, 13u}, {33u, 17u}, {64u, 64u}, {257u, 129u}, {300u, 200u}, {3840u, 2160u}, {16384u, 16384u},
                                      {1u << 28, 1u}};
        for (const auto& f : frames)
            for (uint32_t levels : {1u, 3u, 8u}) {
                const RtGlare g{0.25f, 0.5f, 0.0f, levels};
                const GlarePlan pl = glare_plan(f[0], f[1], g);
                CHECK(pl.levels == glare_levels(f[0], f[1], levels) && pl.levels <= levels);
                struct Region {
                    size_t at, bytes;
                };
                std::vector<Region> rs;
                rs.push_back({pl.out, (size_t)f[0] * f[1] * RT_GLARE_RGB_BYTES});
                for (uint32_t l = 1u; l <= pl.levels; ++l) {
                    CHECK(pl.lv[l].npix == (uint64_t)pl.lv[l].nx * pl.lv[l].rows && pl.lv[l].npix >= 1u && pl.lv[l].w > 0.0f);
                    rs.push_back({pl.lv[l].d, (size_t)pl.lv[l].npix * RT_GLARE_RGB_BYTES});
                    rs.push_back({pl.lv[l].u, (size_t)pl.lv[l].npix * RT_GLARE_RGB_BYTES});
                }
                for (size_t i = 0; i < rs.size(); ++i) {
                    CHECK(rs[i].at % RT_GLARE_ALIGN == 0u && rs[i].at + rs[i].bytes <= pl.total);
                    for (size_t j = 0; j < i; ++j) CHECK(rs[i].at >= rs[j].at + rs[j].bytes || rs[j].at >= rs[i].at + rs[i].bytes);
                }
                // the pyramid adds less than the image itself: d and u together at most 2 (1/4 + 1/16 + ..) of it, plus the rounding up of odd sides
                if ((uint64_t)f[0] * f[1] >= 4096u && f[0] > 16u && f[1] > 16u) CHECK(pl.total < 2u * rs[0].bytes);
            }
    }
    section("layout");
    std::printf("ok\n");
    return 0;
}
