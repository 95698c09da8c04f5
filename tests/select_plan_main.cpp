// The GPU-free arithmetic of "Selected strength" (csrc/rt_select_plan.h) as a stand-alone program: built with AddressSanitizer + UBSan by
// tests/test_select_host.py and run without a GPU.  It prints one line per section — its name and the number of checks made — and "ok";
// a failed check prints what failed and ends the program with status 1.
#include "rt_select_plan.h"

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
    // ---- rt_select_check: the defaults, NULL, and every edge of every range
    const RtSelect def = select_defaults();
    CHECK(select_invalid(nullptr) == nullptr && select_invalid(&def) == nullptr);
    CHECK(def.n_strengths == 3u && def.strength[0] == 0.7f && def.strength[1] == 1.0f && def.strength[2] == 1.4f);
    CHECK(def.radius == 5u && def.patch == 1u && def.error_radius == 0u && def.blend_radius == 1u && def.reserved == 0u);
    const RtSelect good{4u, {0.45f, 0.7f, 1.0f, 1.4f}, 5u, 1u, 2u, 1u, 0u}; // four candidates: every entry is looked at
    CHECK(select_invalid(&good) == nullptr);
    for (uint32_t K = 0; K <= 6u; ++K) {
        RtSelect s = good;
        s.n_strengths = K;
        CHECK((select_invalid(&s) == nullptr) == (K >= 2u && K <= RT_SELECT_MAX));
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (uint32_t K = 2; K <= RT_SELECT_MAX; ++K)
        for (uint32_t j = 0; j < RT_SELECT_MAX; ++j)
            for (float bad : {0.0f, -1.0f, inf, nan}) {
                RtSelect s = good;
                s.n_strengths = K, s.strength[j] = bad;
                CHECK((select_invalid(&s) == nullptr) == (j >= K)); // the entries past K are not looked at
            }
    {
        RtSelect s = good;
        s.strength[1] = s.strength[0]; // equal: not strictly increasing
        CHECK(select_invalid(&s) != nullptr);
        s.strength[1] = 0.3f; // decreasing
        CHECK(select_invalid(&s) != nullptr);
        s = good, s.n_strengths = 2u, s.strength[2] = 0.1f, s.strength[3] = 0.05f; // past K: anything
        CHECK(select_invalid(&s) == nullptr);
    }
    for (uint32_t R = 0; R <= RT_DENOISE_MAX_RADIUS + 1u; ++R) {
        RtSelect s = good;
        s.radius = R;
        CHECK((select_invalid(&s) == nullptr) == (R >= 1u && R <= RT_DENOISE_MAX_RADIUS));
    }
    for (uint32_t F = 0; F <= RT_DENOISE_MAX_PATCH + 1u; ++F) {
        RtSelect s = good;
        s.patch = F;
        CHECK((select_invalid(&s) == nullptr) == (F <= RT_DENOISE_MAX_PATCH));
    }
    for (uint32_t w = 0; w <= RT_SELECT_MAX_WINDOW + 1u; ++w) {
        RtSelect s = good;
        s.error_radius = w;
        CHECK((select_invalid(&s) == nullptr) == (w <= RT_SELECT_MAX_WINDOW));
        s = good, s.blend_radius = w;
        CHECK((select_invalid(&s) == nullptr) == (w <= RT_SELECT_MAX_WINDOW));
    }
    {
        RtSelect s = good;
        s.reserved = 1u;
        CHECK(select_invalid(&s) != nullptr);
    }
    section("check");

    // ---- the windows: every tile entry of every workgroup names a pixel of the image, clamped per axis, and the tile fits its LDS array
    for (uint32_t halo = 0; halo <= RT_SELECT_MAX_WINDOW; ++halo) {
        CHECK(select_side(halo) == 16u + 2u * halo && select_side(halo) <= RT_SEL_SIDE_MAX);
        CHECK(select_window(halo) == (2u * halo + 1u) * (2u * halo + 1u));
        for (uint32_t n : {1u, 3u, 16u, 17u, 70u}) {
            const uint32_t blocks = (n + RT_SEL_TILE - 1u) / RT_SEL_TILE;
            for (uint32_t b = 0; b < blocks; ++b)
                for (uint32_t l = 0; l < select_side(halo); ++l) {
                    const long want = (long)b * 16 + (long)l - (long)halo;
                    const uint32_t got = select_clamp(b, l, halo, n);
                    CHECK(got < n && (long)got == (want < 0 ? 0 : want >= (long)n ? (long)n - 1 : want));
                }
        }
    }
    CHECK(select_clamp(0x0FFFFFF0u, 23u, 4u, 0xFFFFFFFFu) == 0xFFFFFF13u && select_clamp(0x0FFFFFFFu, 23u, 4u, 0xFFFFFFFFu) == 0xFFFFFFFEu); // (64-bit inside: nothing wraps)
    section("windows");

    // ---- the layout: regions disjoint, in order, aligned to 16 B, each as large as its plane
    for (uint64_t npix : {1ull, 6ull, 255ull, 257ull, 1920ull * 1080ull, 1ull << 28})
        for (uint32_t K = 2; K <= RT_SELECT_MAX; ++K) {
            const SelectLayout l = select_layout(npix, K);
            std::vector<std::pair<size_t, size_t>> r; // (offset, bytes) in the order of the layout
            r.push_back({l.partials, (size_t)l.n_partials * sizeof(SelectPartial)});
            r.push_back({l.info, sizeof(RtSelectInfo)});
            for (int h = 0; h < 2; ++h) r.push_back({l.c[h], (size_t)npix * 12u});
            for (int h = 0; h < 2; ++h) r.push_back({l.yv[h], (size_t)npix * 8u});
            r.push_back({l.cnt, (size_t)npix * 4u});
            for (int h = 0; h < 2; ++h)
                for (uint32_t j = 0; j < K; ++j) r.push_back({l.f[h][j], (size_t)npix * 12u});
            for (uint32_t j = 0; j < K; ++j) r.push_back({l.out_j[j], (size_t)npix * 12u});
            for (uint32_t j = 0; j < K; ++j) r.push_back({l.e_j[j], (size_t)npix * 4u});
            r.push_back({l.est, (size_t)npix * 4u});
            r.push_back({l.out, (size_t)npix * 12u});
            r.push_back({l.index, (size_t)npix});
            CHECK(l.n_partials == (npix + 255u) / 256u && r[0].first == 0u);
            for (size_t k = 0; k < r.size(); ++k) {
                CHECK(r[k].first % 16u == 0u);
                const size_t end = k + 1 < r.size() ? r[k + 1].first : l.total;
                CHECK(r[k].first + r[k].second <= end && end - (r[k].first + r[k].second) < 16u);
            }
            CHECK(l.total <= npix * (40u * K + 61u) + 64u * l.n_partials + 16u * 20u);
        }
    CHECK(sizeof(RtSelect) == 40u && sizeof(RtSelectInfo) == 72u && sizeof(SelectPartial) == 64u);
    section("layout");
    std::printf("ok\n");
    return 0;
}
