// The host-side frame arithmetic (csrc/rt_frame_plan.h) as a stand-alone program: built with AddressSanitizer + UBSan by
// tests/test_frame_plan_host.py and run without a GPU (no HIP runtime call).  Every section holds the header against brute force —
// regions laid out by hand, chunks dealt one by one, linear searches, integer division — and prints
//   <section> <checks made>
// A check that does not hold prints FAILED and ends the program with status 1.
#include "rt_frame_plan.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

using namespace rt;

namespace {

int g_bad = 0;
unsigned long long g_checks = 0;
#define EXPECT(cond, ...)                                                        \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) {                                                           \
            if (++g_bad <= 20) std::printf("FAILED %s: ", #cond), std::printf(__VA_ARGS__), std::printf("\n"); \
        }                                                                        \
    } while (0)
void section(const char* name) {
    std::printf("%s %llu\n", name, g_checks);
    if (g_checks == 0) ++g_bad; // (a section that checked nothing is a broken program)
    g_checks = 0;
}

const uint32_t NQS[] = {1u, 7u, 8u, 9u, 2048u};
const unsigned long long SLOT_MAX = 0xFFFFFF00ull; // the most rays of a slice: (n + 255) / 256 stays within 32 bits

// what the kernels store per ray and per path (rt_kernels.h: the 32 B a / b record, the c record, the hit record, the radiance slot)
void check_work_layout() {
    for (size_t n_queue : {(size_t)256, (size_t)512, (size_t)256 * 2048, (size_t)256 * 2049})
        for (size_t n_paths : {(size_t)1, (size_t)255, (size_t)256, (size_t)257, n_queue}) {
            const WorkLayout w = work_layout(n_queue, n_paths);
            std::vector<std::pair<size_t, size_t>> regions; // (offset, bytes stored)
            for (int k = 0; k < 2; ++k) {
                if (RT_QSTRIDE == 2u) {
                    regions.push_back({w.q_ab[k], n_queue * 32u}); // ray i: a at 32 i, b at 32 i + 16
                    EXPECT(w.q_b[k] == w.q_ab[k] + 16u, "queue %d", k);
                } else {
                    regions.push_back({w.q_ab[k], n_queue * 16u});
                    regions.push_back({w.q_b[k], n_queue * 16u});
                }
                regions.push_back({w.q_c[k], n_queue * 8u});
            }
            regions.push_back({w.qhit, n_queue * 8u});
            regions.push_back({w.rad, n_paths * RT_RAD_FLOATS * 4u});
            std::sort(regions.begin(), regions.end());
            for (size_t r = 0; r < regions.size(); ++r) {
                const size_t end = r + 1 < regions.size() ? regions[r + 1].first : w.total;
                EXPECT(regions[r].first % 256u == 0u, "n_queue %zu n_paths %zu region %zu", n_queue, n_paths, r);
                EXPECT(regions[r].first + regions[r].second <= end, "n_queue %zu n_paths %zu region %zu", n_queue, n_paths, r);
            }
        }
    section("work_layout");
}

void check_shard_cap() {
    for (uint32_t nq : NQS)
        for (uint64_t n64 : {1ull, 255ull, 256ull, 257ull, 256ull * nq - 1u, 256ull * nq, 256ull * nq + 1u, SLOT_MAX}) {
            const uint32_t n_max = (uint32_t)n64;
            const uint32_t cap = shard_cap(nq, n_max);
            // the 256-ray chunks of the slice dealt to the shards one by one: chunk c goes to shard c % nq
            std::vector<uint64_t> held(nq, 0);
            for (uint64_t c = 0; c < (n64 + 255u) / 256u; ++c) held[c % nq] += 256u;
            const uint64_t fullest = *std::max_element(held.begin(), held.end());
            EXPECT(cap % 256u == 0u, "nq %u n_max %u", nq, n_max);
            EXPECT((uint64_t)nq * cap >= n64, "nq %u n_max %u", nq, n_max);
            EXPECT(cap == fullest, "nq %u n_max %u: cap %u, fullest shard %llu", nq, n_max, cap, (unsigned long long)fullest);
            EXPECT(cap == (((n64 + 255u) / 256u + nq - 1u) / nq) * 256u, "nq %u n_max %u", nq, n_max);
            const size_t bytes = slice_bytes(nq, n_max, 1u);
            EXPECT(bytes == work_layout((size_t)nq * cap, n_max).total, "nq %u n_max %u", nq, n_max);
            EXPECT(bytes >= 100ull * n64, "nq %u n_max %u: %zu B", nq, n_max, bytes); // (slice_fit starts its search from this)
        }
    section("shard_cap");
}

void check_slice_fit() {
    for (uint32_t npix : {1u, 63u, 64u, 1000u})
        for (uint32_t nq : NQS)
            for (uint32_t sc_max : {1u, 5u, 64u}) {
                std::vector<size_t> sweep{0u, 1u, 99u, 100u};
                for (uint32_t sc = 1; sc <= sc_max; ++sc) // every size at which the answer can change, and its neighbours
                    for (size_t b : {slice_bytes(nq, npix, sc) - 1u, slice_bytes(nq, npix, sc), slice_bytes(nq, npix, sc) + 1u}) sweep.push_back(b);
                sweep.push_back(slice_bytes(nq, npix, sc_max) + 4096u);
                for (size_t bytes : sweep) {
                    uint32_t best = 0;
                    for (uint32_t sc = 1; sc <= sc_max; ++sc)
                        if (slice_bytes(nq, npix, sc) <= bytes) best = sc;
                    const uint32_t got = slice_fit(nq, npix, bytes, sc_max);
                    EXPECT(got == best, "npix %u nq %u sc_max %u bytes %zu: %u, linear search %u", npix, nq, sc_max, bytes, got, best);
                }
            }
    section("slice_fit");
}

void check_plan() {
    const uint64_t NPIX[] = {1u, 64u * 36u, 1920u * 1080u, 1ull << 24, 1ull << 31, SLOT_MAX, SLOT_MAX + 1u};
    const uint32_t SPP[] = {1u, 3u, 1024u, 1u << 20, 1u << 21, 0xFFFFFFFFu};
    const uint32_t SPP_SLICE[] = {0u, 1u, 7u, (1u << 20) + 1u, 0xFFFFFFFFu};
    const size_t FREE[] = {0u, (size_t)1 << 20, (size_t)1 << 30, (size_t)300 << 30, SIZE_MAX};
    const size_t MAPPED[] = {0u, (size_t)1 << 30};
    const size_t BASE[] = {0u, 4096u, (size_t)1 << 28};
    for (uint64_t npix64 : NPIX)
        for (uint32_t spp : SPP)
            for (uint32_t spp_slice : SPP_SLICE)
                for (uint32_t nq : {8u, 2048u})
                    for (size_t free_b : FREE)
                        for (size_t mapped : MAPPED)
                            for (size_t base : BASE) {
                                RtParams p{};
                                p.spp = spp, p.spp_slice = spp_slice;
                                SlicePlan pl{};
                                const bool ok = plan_slice_size(p, npix64, nq, free_b, mapped, base, pl);
                                // refused only when not even one sample per pixel stays within the slot arithmetic
                                EXPECT(ok == (npix64 <= SLOT_MAX), "npix %llu", (unsigned long long)npix64);
                                if (!ok) continue;
                                const uint32_t S = pl.S_cap, npix = (uint32_t)npix64;
                                EXPECT(S >= 1u && S <= spp && S <= (1u << 20), "npix %llu spp %u slice %u: S %u", (unsigned long long)npix64, spp, spp_slice, S);
                                EXPECT((uint64_t)S * npix64 <= SLOT_MAX, "npix %llu spp %u slice %u: S %u", (unsigned long long)npix64, spp, spp_slice, S);
                                EXPECT(pl.by_library == (spp_slice == 0u), "slice %u", spp_slice);
                                EXPECT(pl.want_bytes == base + slice_bytes(nq, npix, S), "npix %llu S %u", (unsigned long long)npix64, S);
                                if (spp_slice != 0u) { // the caller's size, held to spp and the slot arithmetic only
                                    const uint64_t want = std::min<uint64_t>(std::min<uint64_t>(spp_slice, spp), std::min<uint64_t>(1u << 20, SLOT_MAX / npix64));
                                    EXPECT(S == want, "npix %llu spp %u slice %u: S %u", (unsigned long long)npix64, spp, spp_slice, S);
                                } else if (free_b != SIZE_MAX) { // never more than half of what the device has free, if one sample per pixel allows it
                                    const size_t half = (free_b + mapped) / 2u;
                                    if (base + slice_bytes(nq, npix, 1u) <= half)
                                        EXPECT(pl.want_bytes <= half, "npix %llu spp %u free %zu mapped %zu base %zu: S %u", (unsigned long long)npix64, spp, free_b, mapped, base, S);
                                }
                            }
    section("plan_slice_size");
}

void check_pixel_order_and_shards() {
    for (uint32_t po : {0u, 1u, 2u})
        for (bool general : {false, true})
            for (uint32_t nx : {1u, 7u, 8u, 9u, 16u, 64u, 1920u})
                for (uint32_t rows : {0u, 1u, 7u, 8u, 9u, 36u, 135u}) {
                    const PixelOrder o = pixel_order(po, general, nx, rows);
                    const uint32_t npix = nx * rows;
                    const bool may_tile = nx % 8u == 0u && rows >= 8u;
                    EXPECT(o.tile_pixels <= npix && o.tile_pixels % nx == 0u, "po %u nx %u rows %u", po, nx, rows);
                    EXPECT(may_tile || (o.tiles_per_row == 0u && o.tile_pixels == 0u), "po %u nx %u rows %u", po, nx, rows);
                    EXPECT((o.tiles_per_row != 0u) == (may_tile && (po == 2u || (po == 0u && !general))), "po %u general %d nx %u rows %u", po, (int)general, nx, rows);
                    EXPECT(o.tiles_per_row == 0u || (o.tiles_per_row == nx / 8u && o.tile_pixels == nx * (rows - rows % 8u)), "po %u nx %u rows %u", po, nx, rows);
                    // the order the kernels enumerate (local_of_pixel, rt_kernels.h) names every pixel of the frame exactly once
                    std::vector<uint8_t> seen(npix, 0);
                    bool once = true;
                    for (uint32_t lj = 0; lj < rows; ++lj)
                        for (uint32_t i = 0; i < nx; ++i) {
                            const uint32_t pl = local_of_pixel(nx, o.tiles_per_row, o.tile_pixels, i, lj);
                            once = once && pl < npix && !seen[pl];
                            if (pl < npix) seen[pl] = 1;
                        }
                    EXPECT(once, "po %u general %d nx %u rows %u", po, (int)general, nx, rows);
                }
    for (uint32_t ny : {1u, 7u, 8u, 9u, 36u})
        for (uint32_t band : {0u, 1u, 4u, 8u}) // (0: the default, 1)
            for (uint32_t count : {0u, 1u, 2u, 3u}) {
                uint32_t sum = 0;
                for (uint32_t id = 0; id < std::max(count, 1u); ++id) {
                    RtParams p{};
                    p.nx = 5, p.ny = ny, p.shard_band = band, p.shard_count = count, p.shard_id = id;
                    const ShardGeom g = shard_geom(p);
                    uint32_t mine = 0; // image rows j with (j / band) % count == id
                    for (uint32_t j = 0; j < ny; ++j) mine += (j / std::max(band, 1u)) % std::max(count, 1u) == id;
                    EXPECT(g.rows == mine && g.npix64 == 5ull * mine, "ny %u band %u count %u id %u: %u rows, %u by counting", ny, band, count, id, g.rows, mine);
                    EXPECT(g.band == std::max(band, 1u) && g.count == std::max(count, 1u) && g.id == id, "ny %u band %u count %u id %u", ny, band, count, id);
                    EXPECT(g.rows == shard_rows(ny, g.band, g.count, id), "ny %u band %u count %u id %u", ny, band, count, id);
                    sum += g.rows;
                }
                EXPECT(sum == ny, "ny %u band %u count %u: %u", ny, band, count, sum);
            }
    section("pixel_order_and_shard_rows");
}

// x / d through the kernels' own udiv_inv with the header's reciprocal, against integer division
void check_division(uint32_t x, uint32_t d, float inv) {
    const uint32_t estimate = (uint32_t)((float)x * inv);
    uint32_t rem = ~0u;
    const uint32_t q = udiv_inv(x, d, inv, rem);
    EXPECT(estimate <= x / d, "x %u d %u: estimate %u", x, d, estimate);
    EXPECT(q == x / d && rem == x % d, "x %u d %u: %u rem %u", x, d, q, rem);
}
void check_udiv_inv() {
    std::mt19937_64 rng(20240607u);
    for (uint64_t d64 : {1ull, 2ull, 3ull, 7ull, 8ull, 255ull, 256ull, 257ull, 1920ull, 4095ull, 65537ull, (1ull << 20) - 1u, 1ull << 20, (1ull << 21) + 1u,
                         (1ull << 24) + 1u, SLOT_MAX}) {
        const uint32_t d = (uint32_t)d64;
        const float inv = udiv_reciprocal(d);
        const uint64_t q_max = std::min<uint64_t>((1u << 21) - 1u, SLOT_MAX / d64);
        std::vector<uint64_t> qs{0u, q_max};
        for (int k = 0; k < 4000; ++k) qs.push_back(rng() % (q_max + 1u));
        for (uint64_t q : qs)
            for (uint64_t r : {(uint64_t)0, (uint64_t)1, (uint64_t)(d64 - 1u)}) {
                const uint64_t x = q * d64 + r;
                if (r < d64 && x <= SLOT_MAX) check_division((uint32_t)x, d, inv);
            }
    }
    section("udiv_inv");
    // ... and with the reciprocals of whole frames: slot -> (sample, local pixel) -> (row, column) -> (band, row in band), as
    // path_key_of_slot and gen_primary undo them
    for (uint32_t count : {1u, 3u}) {
        RtParams p{};
        p.nx = 1920, p.ny = 1080, p.spp = 64, p.seed = 0x123456789ull, p.shard_band = 4, p.shard_count = count, p.shard_id = count - 1u;
        const ShardGeom sh = shard_geom(p);
        const PixelOrder po = pixel_order(1u, false, p.nx, sh.rows);
        const GenParams gp = frame_gen_params(RtCamera{}, p, sh, 2048u, po);
        EXPECT(gp.npix == sh.rows * p.nx && gp.nx == p.nx && gp.ny == p.ny && gp.nq == 2048u, "count %u", count);
        EXPECT(gp.shard_band == 4u && gp.shard_count == count && gp.shard_id == count - 1u, "count %u", count);
        EXPECT(gp.seed_lo == 0x23456789u && gp.seed_hi == 0x1u && gp.tiles_per_row == 0u && gp.lists == nullptr, "count %u", count);
        const uint64_t n_slots = (uint64_t)gp.npix * p.spp;
        for (int k = 0; k < 20000; ++k) {
            const uint32_t slot = k == 0 ? 0u : k == 1 ? (uint32_t)(n_slots - 1u) : (uint32_t)(rng() % n_slots);
            check_division(slot, gp.npix, gp.inv_npix);
            check_division(slot % gp.npix, gp.nx, gp.inv_nx);
            check_division(slot % gp.npix / gp.nx, gp.shard_band, gp.inv_band);
        }
    }
    const PixelOrder tiles = pixel_order(2u, false, 1920u, 1080u);
    RtParams p{};
    p.nx = 1920, p.ny = 1080;
    const GenParams gt = frame_gen_params(RtCamera{}, p, shard_geom(p), 2048u, tiles);
    for (uint32_t pl = 0; pl < tiles.tile_pixels; pl += 61u) check_division(pl >> 6, gt.tiles_per_row, gt.inv_tpr);
    section("frame_gen_params");
}

} // namespace

int main() {
    check_work_layout();
    check_shard_cap();
    check_slice_fit();
    check_plan();
    check_pixel_order_and_shards();
    check_udiv_inv();
    if (g_bad) std::printf("FAILED: %d checks\n", g_bad);
    else std::printf("ok\n");
    return g_bad ? 1 : 0;
}
