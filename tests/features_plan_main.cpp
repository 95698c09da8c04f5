// The GPU-free arithmetic of the first-hit features (csrc/rt_features_plan.h, and the features' row in csrc/rt_accum_planes.h) as a
// stand-alone program: built with AddressSanitizer + UBSan by tests/test_features_host.py and run without a GPU.  It prints one line per
// section — its name and the number of checks made — and "ok"; a failed check prints what failed and ends the program with status 1.
#include "rt_accum_planes.h"
#include "rt_features_plan.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <cstdlib>
#include <cstring>
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
    // ---- rt_features_check: each refusal
    CHECK(features_invalid(nullptr) != nullptr);
    for (uint32_t stride = 0; stride <= 70u; ++stride) {
        RtFeatures f{stride, 0u};
        CHECK((features_invalid(&f) == nullptr) == (stride >= 1u && stride <= 64u));
        f.reserved = 1u;
        CHECK(features_invalid(&f) != nullptr);
    }
    for (const uint32_t stride : {65u, 0x80000000u, 0xFFFFFFFFu}) {
        const RtFeatures f{stride, 0u};
        CHECK(features_invalid(&f) != nullptr);
    }
    section("features_check");

    // ---- rt_accum_features_check: each refusal
    {
        RtFeaturePixel px[2] = {};
        RtAccumFeatures good{};
        good.nx = 2u, good.rows = 1u, good.first_sample = 3u, good.done = 4u, good.frame_id = 9u, good.features = RtFeatures{2u, 0u}, good.plane = px;
        CHECK(accum_features_invalid(nullptr) != nullptr);
        CHECK(accum_features_invalid(&good) == nullptr);
        RtAccumFeatures b = good;
        b.reserved[0] = 1u;
        CHECK(accum_features_invalid(&b) != nullptr);
        b = good, b.reserved[1] = 1u;
        CHECK(accum_features_invalid(&b) != nullptr);
        b = good, b.plane = nullptr;
        CHECK(accum_features_invalid(&b) != nullptr);
        b = good, b.first_sample = 0xFFFFFFFFu, b.done = 1u;
        CHECK(accum_features_invalid(&b) != nullptr);
        b = good, b.first_sample = 0xFFFFFFFEu, b.done = 1u;
        CHECK(accum_features_invalid(&b) == nullptr);
        b = good, b.features.stride = 0u;
        CHECK(accum_features_invalid(&b) != nullptr);
        b = good, b.features.stride = 65u;
        CHECK(accum_features_invalid(&b) != nullptr);
        b = good, b.features.reserved = 7u;
        CHECK(accum_features_invalid(&b) != nullptr);
    }
    section("accum_features_check");

    // ---- rt_feature_guide_check: each refusal
    {
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        const RtFeatureGuide good{0.6f, 0.6f, 0.6f, 1e-3f, 1e-3f, 1e-3f, 7u, 0u, {0u, 0u}};
        CHECK(feature_guide_invalid(nullptr) != nullptr);
        CHECK(feature_guide_invalid(&good) == nullptr);
        float RtFeatureGuide::*const ks[3] = {&RtFeatureGuide::k_albedo, &RtFeatureGuide::k_normal, &RtFeatureGuide::k_depth};
        float RtFeatureGuide::*const taus[3] = {&RtFeatureGuide::tau_albedo, &RtFeatureGuide::tau_normal, &RtFeatureGuide::tau_depth};
        for (int f = 0; f < 3; ++f) {
            for (const float bad : {0.0f, -0.5f, nan, inf, -inf}) {
                RtFeatureGuide b = good;
                b.*ks[f] = bad;
                CHECK(feature_guide_invalid(&b) != nullptr);
            }
            for (const float bad : {-1e-9f, nan, inf, -inf}) {
                RtFeatureGuide b = good;
                b.*taus[f] = bad;
                CHECK(feature_guide_invalid(&b) != nullptr);
            }
            RtFeatureGuide b = good;
            b.*taus[f] = 0.0f, b.*ks[f] = std::numeric_limits<float>::min();
            CHECK(feature_guide_invalid(&b) == nullptr);
        }
        for (uint32_t use = 0; use <= 7u; ++use) {
            RtFeatureGuide b = good;
            b.use_mask = use, b.demodulate = use;
            CHECK(feature_guide_invalid(&b) == nullptr);
        }
        for (const uint32_t use : {8u, 15u, 0x80000001u}) {
            RtFeatureGuide b = good;
            b.use_mask = use;
            CHECK(feature_guide_invalid(&b) != nullptr);
        }
        for (int k = 0; k < 2; ++k) {
            RtFeatureGuide b = good;
            b.reserved[k] = 1u;
            CHECK(feature_guide_invalid(&b) != nullptr);
        }
        CHECK(features_guide_bytes(800u) == 800u * 40u);
    }
    section("feature_guide_check");

    // ---- which samples of a window contribute: every stride against brute force, first samples that are no multiple of the stride, windows
    // that hold none, windows at the end of the 32-bit range
    for (uint32_t stride = 1; stride <= 64u; ++stride) {
        for (const uint32_t i0 : {0u, 1u, 2u, 5u, 63u, 64u, 65u, 1000u, 0xFFFFFF00u, 0xFFFFFFF0u}) {
            for (uint32_t n = 0; n <= 140u; ++n) {
                if ((uint64_t)i0 + n > (1ull << 32)) break;
                uint32_t want = 0;
                uint64_t first = ~0ull;
                for (uint64_t s = i0; s < (uint64_t)i0 + n; ++s)
                    if (s % stride == 0u) {
                        if (!want) first = s;
                        ++want;
                    }
                CHECK(features_in_window(i0, n, stride) == want);
                if (want) CHECK(features_first(i0, stride) == first);
                else CHECK(features_first(i0, stride) >= (uint64_t)i0 + n);
            }
        }
        // a window cut in two contributes what the whole does
        for (uint32_t cut = 0; cut <= 100u; ++cut) CHECK(features_in_window(7u, cut, stride) + features_in_window(7u + cut, 100u - cut, stride) == features_in_window(7u, 100u, stride));
    }
    CHECK(features_in_window(1u, 2u, 3u) == 0u && features_in_window(4u, 2u, 3u) == 0u && features_in_window(3u, 1u, 3u) == 1u);
    CHECK(features_in_window(0xFFFFFFFFu, 1u, 1u) == 1u && features_in_window(0xFFFFFFFFu, 1u, 64u) == 0u && features_in_window(0xFFFFFFC0u, 64u, 64u) == 1u);
    section("windows");

    // ---- buffer sizes, and the record as one PlaneTable row of four 16 B parts
    CHECK(sizeof(RtFeaturePixel) == 64u && RT_FEATURES_PIXEL_BYTES == 64u);
    for (const uint64_t npix : {0ull, 1ull, 7ull, 800ull, 1920ull * 1080ull}) {
        CHECK(features_buffer_bytes(npix) == npix * 64u);
        CHECK(features_read_bytes(npix) == npix * 44u);
        for (uint32_t q = 0; q < 4u; ++q) CHECK(features_quarter_offset(npix, q) == npix * 16u * q);
        CHECK(features_quarter_offset(npix, 3u) + npix * 16u == features_buffer_bytes(npix));
    }
    {
        const uint64_t npix = 6;
        std::vector<RtFeaturePixel> host(npix);
        std::vector<unsigned char> local(features_buffer_bytes(npix));
        RtAccumFeatures fs{};
        fs.plane = host.data();
        PlaneTable t = features_planes(fs, local.data());
        CHECK(t.n == 1u && t.row[0].elem_bytes == 16u && t.row[0].parts == 4u && t.row[0].host == host.data() && t.row[0].local == local.data());
        CHECK(plane_bytes(t.row[0], npix) == npix * sizeof(RtFeaturePixel));
        CHECK(planes_place(t, npix) == npix * sizeof(RtFeaturePixel) && t.row[0].stage == 0u);
        // the move k_planes_move makes with such a row, on the host: part k of local pixel lp <-> quarter k of the record of image pixel p
        for (uint64_t p = 0; p < npix; ++p) {
            host[p].albedo[0] = (float)p, host[p].n_f = (uint32_t)(10u + p), host[p].normal[2] = -(float)p, host[p].n_h = (uint32_t)(20u + p);
            host[p].a2 = 1.5 * (double)p, host[p].n2 = 2.5 * (double)p, host[p].z1 = 3.5 * (double)p, host[p].z2 = 4.5 * (double)p;
        }
        for (uint64_t p = 0; p < npix; ++p)
            for (uint32_t part = 0; part < 4u; ++part)
                std::memcpy(local.data() + features_quarter_offset(npix, part) + 16u * p, reinterpret_cast<const unsigned char*>(&host[p]) + 16u * part, 16u);
        for (uint64_t p = 0; p < npix; ++p) {
            uint32_t n_f, n_h;
            double z2;
            std::memcpy(&n_f, local.data() + features_quarter_offset(npix, 0u) + 16u * p + 12u, 4u);
            std::memcpy(&n_h, local.data() + features_quarter_offset(npix, 1u) + 16u * p + 12u, 4u);
            std::memcpy(&z2, local.data() + features_quarter_offset(npix, 3u) + 16u * p + 8u, 8u);
            CHECK(n_f == 10u + p && n_h == 20u + p && z2 == 4.5 * (double)p);
        }
    }
    section("sizes");
    std::printf("ok\n");
    return 0;
}
