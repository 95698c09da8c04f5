// The GPU-free arithmetic of the multi-scale filter (csrc/rt_multiscale_plan.h) as a stand-alone program: built with AddressSanitizer +
// UBSan by tests/test_denoise_multiscale_host.py and run without a GPU.  It prints one line per section — its name and the number of
// checks made — and "ok"; a failed check prints what failed and ends the program with status 1.
#include "rt_multiscale_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
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

// Every region of the plan with its size: inside the buffer, aligned, and no two that hold bytes overlap (o of the coarsest level IS f).
static void check_regions(const rt::MultiscalePlan& pl) {
    using namespace rt;
    std::vector<std::pair<size_t, size_t>> spans; // (offset, bytes) of the regions that hold something
    for (uint32_t s = 0; s < pl.levels; ++s) {
        const MultiscaleLevel& l = pl.lv[s];
        const size_t rgb = (size_t)l.npix * RT_MS_RGB_BYTES, guide = (size_t)l.npix * pl.planes * RT_MS_PLANE_BYTES;
        const bool last = s + 1u == pl.levels;
        for (size_t off : {l.c, l.guide, l.f, l.e, l.o}) CHECK(off % RT_MS_ALIGN == 0u);
        if (pl.planes == 1u) spans.push_back({l.c, rgb});
        else CHECK(l.c == l.guide);
        spans.push_back({l.guide, guide});
        spans.push_back({l.f, rgb});
        if (s) spans.push_back({l.e, rgb});
        if (last) CHECK(l.o == l.f);
        else spans.push_back({l.o, rgb});
    }
    std::sort(spans.begin(), spans.end());
    for (size_t k = 0; k < spans.size(); ++k) {
        CHECK(spans[k].second > 0u);
        CHECK(spans[k].first + spans[k].second <= (k + 1u < spans.size() ? spans[k + 1u].first : pl.total));
    }
}

int main() {
    using namespace rt;
    // ---- the level sizes: halves rounded up, a side of 1 stays 1, nothing wraps
    for (uint32_t side = 1u; side <= 70u; ++side) CHECK(multiscale_half(side) == (side + 1u) / 2u);
    CHECK(multiscale_half(1u) == 1u && multiscale_half(0xFFFFFFFFu) == 0x80000000u && multiscale_half(0xFFFFFFFEu) == 0x7FFFFFFFu);
    section("sizes");

    // ---- multiscale_invalid: each refusal
    {
        RtMultiscale good{2u, RT_DENOISE_GUIDE_LUMINANCE, {0u, 0u}};
        CHECK(multiscale_invalid(&good) == nullptr);
        CHECK(multiscale_invalid(nullptr) != nullptr);
        for (uint32_t L = 0u; L <= RT_DENOISE_MAX_LEVELS + 1u; ++L) {
            RtMultiscale m = good;
            m.levels = L;
            CHECK((multiscale_invalid(&m) == nullptr) == (L >= 1u && L <= RT_DENOISE_MAX_LEVELS));
        }
        RtMultiscale m = good;
        m.guide = RT_DENOISE_GUIDE_CHANNELS;
        CHECK(multiscale_invalid(&m) == nullptr);
        m.guide = 2u;
        CHECK(multiscale_invalid(&m) != nullptr);
        m.guide = 0xFFFFFFFFu;
        CHECK(multiscale_invalid(&m) != nullptr);
        for (int k = 0; k < 2; ++k) {
            m = good, m.reserved[k] = 1u;
            CHECK(multiscale_invalid(&m) != nullptr);
        }
        CHECK(RT_DENOISE_DEFAULT_LEVELS >= 1u && RT_DENOISE_DEFAULT_LEVELS <= RT_DENOISE_MAX_LEVELS);
    }
    section("check");

    // ---- the plan: level sizes, regions disjoint and aligned, at the smallest frame, odd frames, and 2^28 pixels
    const uint32_t frames[][2] = {{1u, 1u}, {2u, 2u}, {3u, 1u}, {1u, 5u}, {37u, 21u}, {35u, 19u}, {1920u, 1080u}, {16384u, 16384u}, {1u << 28, 1u}, {1u, 1u << 28}};
    for (const auto& fr : frames)
        for (uint32_t planes : {1u, 3u})
            for (uint32_t L = 1u; L <= RT_DENOISE_MAX_LEVELS; ++L) {
                const MultiscalePlan pl = multiscale_plan(fr[0], fr[1], L, planes);
                CHECK(pl.levels == L && pl.planes == planes);
                uint32_t nx = fr[0], rows = fr[1];
                uint64_t above = 0;
                for (uint32_t s = 0; s < L; ++s) {
                    CHECK(pl.lv[s].nx == nx && pl.lv[s].rows == rows && pl.lv[s].npix == (uint64_t)nx * rows && pl.lv[s].npix >= 1u);
                    if (s) above += pl.lv[s].npix;
                    nx = (uint32_t)(((uint64_t)nx + 1u) / 2u), rows = (uint32_t)(((uint64_t)rows + 1u) / 2u);
                }
                check_regions(pl);
                // what a pixel of a level takes at the most, and the padding of at most RT_MS_ALIGN - 1 bytes per region
                const uint64_t per_pixel = (planes == 1u ? 12u + 8u : 24u) + 12u + 12u + 12u;
                CHECK(pl.total <= (pl.lv[0].npix + above) * per_pixel + 5u * L * RT_MS_ALIGN);
                if (fr[0] % 8u == 0u && fr[1] % 8u == 0u) CHECK(3u * above <= pl.lv[0].npix); // dyadic sides: 1/4 + 1/16 + 1/64 <= 1/3
            }
    {
        const MultiscalePlan one = multiscale_plan(1u, 1u, RT_DENOISE_MAX_LEVELS, 1u);
        for (uint32_t s = 0; s < RT_DENOISE_MAX_LEVELS; ++s) CHECK(one.lv[s].nx == 1u && one.lv[s].rows == 1u);
        CHECK(one.total == (4u + 5u + 5u + 4u) * RT_MS_ALIGN); // c, guide, f and o; c, guide, f, e and o twice; c, guide, f and e: one pixel each, rounded up
        const MultiscalePlan big = multiscale_plan(16384u, 16384u, RT_DENOISE_MAX_LEVELS, 3u);
        CHECK(big.lv[0].npix == (1ull << 28) && big.lv[3].nx == 2048u && big.lv[3].npix == (1ull << 22));
        CHECK(big.lv[0].guide == 0u && big.lv[0].f == (24ull << 28) && big.lv[0].o == (36ull << 28) && big.lv[1].guide == (48ull << 28));
        CHECK(big.total == (48ull << 28) + (60ull << 26) + (60ull << 24) + (48ull << 22));
        const MultiscalePlan single = multiscale_plan(1920u, 1080u, 1u, 1u);
        CHECK(single.lv[0].o == single.lv[0].f && single.total == 1920ull * 1080ull * 32ull); // (each region a multiple of RT_MS_ALIGN already)
    }
    section("plan");
    std::printf("ok\n");
    return 0;
}
