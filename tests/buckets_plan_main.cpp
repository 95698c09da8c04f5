// The GPU-free arithmetic of the sample buckets (csrc/rt_buckets_plan.h) as a stand-alone program: built with AddressSanitizer + UBSan by
// tests/test_robust_host.py and run without a GPU.  It prints one line per section — its name and the number of checks made — and "ok";
// a failed check prints what failed and ends the program with status 1.
#include "rt_buckets_plan.h"

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
    // ---- n_b against brute force over the absolute indices (64-bit, so that the window may end at 2^32 - 1)
    for (uint32_t M : {3u, 5u, 16u})
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)M - 1, (uint64_t)M, (uint64_t)M + 1, (uint64_t)2 * M + 3})
            for (uint64_t first : {(uint64_t)0, (uint64_t)1, (uint64_t)M - 1, (uint64_t)0xFFFFFFFFull - n}) {
                std::vector<uint32_t> brute(M, 0u);
                for (uint64_t i = first; i < first + n; ++i) ++brute[i % M];
                uint64_t sum = 0;
                for (uint32_t b = 0; b < M; ++b) {
                    CHECK(buckets_count((uint32_t)first, (uint32_t)n, M, b) == brute[b]);
                    sum += buckets_count((uint32_t)first, (uint32_t)n, M, b);
                }
                CHECK(sum == n);
            }
    {
        uint64_t sum = 0; // the whole range: 2^32 - 1 samples from 0
        for (uint32_t b = 0; b < 5u; ++b) sum += buckets_count(0u, 0xFFFFFFFFu, 5u, b);
        CHECK(sum == 0xFFFFFFFFull);
        CHECK(buckets_count(0u, 0xFFFFFFFFu, 5u, 0u) == 858993459u && buckets_count(0u, 0xFFFFFFFFu, 5u, 4u) == 858993459u);
        CHECK(buckets_count(0xFFFFFFFFu, 0xFFFFFFFFu, 16u, 15u) == 0x10000000u); // (no such window exists; the count still forms no sum that wraps)
    }
    section("counts");

    // ---- rt_accum_buckets_check: each refusal, and that no plane is read (the planes are one element long)
    std::vector<float> plane(3);
    RtAccumBuckets good{};
    good.nx = 1000u, good.rows = 1000u, good.first_sample = 3u, good.done = 7u, good.M = 5u, good.frame_id = 42u;
    for (uint32_t b = 0; b < 5u; ++b) good.sum[b] = plane.data();
    CHECK(accum_buckets_invalid(&good) == nullptr);
    CHECK(accum_buckets_invalid(nullptr) != nullptr);
    {
        RtAccumBuckets b = good;
        b.reserved = 1u;
        CHECK(accum_buckets_invalid(&b) != nullptr);
        for (uint32_t M : {0u, 2u, RT_BUCKETS_MAX + 1u}) {
            b = good, b.M = M;
            CHECK(accum_buckets_invalid(&b) != nullptr);
        }
        for (uint32_t k = 0; k < 5u; ++k) {
            b = good, b.sum[k] = nullptr;
            CHECK(accum_buckets_invalid(&b) != nullptr);
        }
        b = good, b.M = 3u; // the pointers past M are not looked at
        CHECK(accum_buckets_invalid(&b) == nullptr);
        b = good, b.M = RT_BUCKETS_MAX;
        CHECK(accum_buckets_invalid(&b) != nullptr);
        for (uint32_t k = 0; k < RT_BUCKETS_MAX; ++k) b.sum[k] = plane.data();
        CHECK(accum_buckets_invalid(&b) == nullptr);
        b = good, b.first_sample = 0xFFFFFFFFu - 7u;
        CHECK(accum_buckets_invalid(&b) == nullptr);
        b.first_sample += 1u;
        CHECK(accum_buckets_invalid(&b) != nullptr);
        b = good, b.nx = 0u, b.rows = 0u, b.done = 0u;
        CHECK(accum_buckets_invalid(&b) == nullptr);
    }
    {
        RtRobust r{RT_ROBUST_GINI, 0u, {0u, 0u}};
        CHECK(robust_invalid(nullptr) == nullptr && robust_invalid(&r) == nullptr);
        r.mode = RT_ROBUST_TRIM, r.trim = 0xFFFFFFFFu;
        CHECK(robust_invalid(&r) == nullptr);
        r.mode = RT_ROBUST_TRIM + 1u;
        CHECK(robust_invalid(&r) != nullptr);
        r.mode = RT_ROBUST_MEDIAN, r.reserved[1] = 1u;
        CHECK(robust_invalid(&r) != nullptr);
    }
    section("check");

    // ---- the layout: M planes, disjoint, 12 M B per pixel
    for (uint64_t npix : {0ull, 1ull, 255ull, 257ull, 1920ull * 1080ull})
        for (uint32_t M : {3u, 5u, 16u}) {
            CHECK(buckets_total(npix, M) == npix * buckets_pixel_bytes(M) && buckets_pixel_bytes(M) == 12u * M);
            for (uint32_t b = 0; b < M; ++b) CHECK(buckets_plane(npix, b) == b * npix * 12u && buckets_plane(npix, b) % 4u == 0u);
        }
    section("layout");
    std::printf("ok\n");
    return 0;
}
