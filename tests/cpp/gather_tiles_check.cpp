// gather_tiles_check.cpp — csrc/gather_tiles.hpp, the work split of pvac_hip_batch_gather, checked on the
// CPU (tests/test_gather_tiles.py builds this with ASan + UBSan): for sigma widths 0, 3 and 128 and count
// vectors that include zeros and the tile boundaries,
//   - the tiles of all ciphers partition every edge row and every layer record exactly once;
//   - the tile -> cipher search agrees with a linear walk, and so does the forward walk of a run;
//   - the runs of all lane groups partition the tiles, for several grids;
//   - the head / body / tail split of the 16-byte path covers every word once and stays inside the range,
//     with 16-byte pieces aligned on both sides, for all four parity combinations.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gather_tiles.hpp"

using namespace pvhip;

static long g_checks = 0;
#define MUST(cond, ...)                                               \
    do {                                                              \
        ++g_checks;                                                   \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);                        \
            std::fprintf(stderr, "\n");                               \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

static void check_batch(const std::vector<uint64_t>& E, const std::vector<uint64_t>& L, uint32_t sw) {
    const gather_geom g = gather_geom_of(sw);
    const size_t n = E.size();
    std::vector<uint64_t> toff(n + 1, 0);
    for (size_t i = 0; i < n; ++i) toff[i + 1] = toff[i] + gather_tiles(E[i], L[i], g);
    const uint64_t ntiles = toff[n];
    std::vector<std::vector<uint8_t>> seenE(n), seenL(n);
    for (size_t i = 0; i < n; ++i) {
        seenE[i].assign(E[i], 0);
        seenL[i].assign(L[i], 0);
    }
    size_t walk = 0;   // the linear walk: the cipher whose tile range holds t
    for (uint64_t t = 0; t < ntiles; ++t) {
        while (toff[walk + 1] <= t) ++walk;
        const uint64_t k = gather_tile_cipher(toff.data(), n, t);
        MUST(k == walk, "sw %u tile %llu: search %llu, walk %zu", sw, (unsigned long long)t, (unsigned long long)k, walk);
        const gather_piece p = gather_piece_of(E[k], L[k], g, t - toff[k]);
        MUST(p.count >= 1 && p.count <= (p.layers ? g.lpt : g.ept), "tile %llu: %llu rows", (unsigned long long)t,
             (unsigned long long)p.count);
        std::vector<uint8_t>& seen = p.layers ? seenL[k] : seenE[k];
        MUST(p.first + p.count <= seen.size(), "tile %llu leaves its cipher", (unsigned long long)t);
        for (uint64_t r = p.first; r < p.first + p.count; ++r) {
            MUST(!seen[r], "row %llu of cipher %llu twice", (unsigned long long)r, (unsigned long long)k);
            seen[r] = 1;
        }
    }
    for (size_t i = 0; i < n; ++i) {
        for (uint8_t s : seenE[i]) MUST(s, "an edge row of cipher %zu is in no tile", i);
        for (uint8_t s : seenL[i]) MUST(s, "a layer record of cipher %zu is in no tile", i);
    }
    // runs: every tile in exactly one group's run, and the kernel's forward walk finds its cipher
    for (uint32_t cus : {1u, 3u, 256u}) {
        for (uint32_t tpb : {1u, 4u}) {
            const uint64_t grid = gather_grid(ntiles, tpb, cus);
            MUST(grid <= (uint64_t)cus * kGatherBlocksPerCu && (ntiles == 0) == (grid == 0), "grid %llu", (unsigned long long)grid);
            const uint64_t groups = grid * tpb;
            uint64_t next = 0;
            for (uint64_t gi = 0; gi < groups; ++gi) {
                uint64_t lo, hi;
                gather_run(ntiles, groups, gi, lo, hi);
                MUST(lo <= hi && hi <= ntiles, "run of group %llu", (unsigned long long)gi);
                if (lo == hi) continue;
                MUST(lo == next, "group %llu starts at %llu, not %llu", (unsigned long long)gi, (unsigned long long)lo,
                     (unsigned long long)next);
                next = hi;
                uint64_t k = gather_tile_cipher(toff.data(), n, lo);
                for (uint64_t t = lo; t < hi; ++t) {
                    while (k + 1 < n && toff[k + 1] <= t) ++k;
                    MUST(toff[k] <= t && t < toff[k + 1], "the forward walk lost tile %llu", (unsigned long long)t);
                }
            }
            MUST(next == ntiles, "the runs end at %llu of %llu", (unsigned long long)next, (unsigned long long)ntiles);
        }
    }
}

static void check_split() {
    for (uint64_t s = 0; s < 4; ++s)
        for (uint64_t d = 0; d < 4; ++d)
            for (uint64_t n = 0; n < 70; ++n) {
                const gather_split p = gather_split_of(1000 + s, 2000 + d, n);
                MUST(p.head + 2 * p.pairs + p.tail == n, "split of %llu words", (unsigned long long)n);
                MUST(p.tail <= 1, "tail");
                if ((s ^ d) & 1) {
                    MUST(p.head == n && !p.pairs && !p.tail, "differing parities move 8 bytes at a time");
                    continue;
                }
                MUST(p.head <= 1, "head");
                if (p.pairs) {   // both sides of every 16-byte piece start at an even word
                    MUST(((2000 + d + p.head) & 1) == 0 && ((1000 + s + p.head) & 1) == 0, "a 16-byte piece at an odd word");
                }
                if (n >= 3) MUST(p.pairs >= 1, "a range of 3 words or more has a 16-byte piece");
                // cover: word w is written once
                std::vector<int> hit(n, 0);
                for (uint64_t w = 0; w < p.head; ++w) ++hit[w];
                for (uint64_t q = 0; q < p.pairs; ++q) {
                    MUST(p.head + 2 * q + 1 < n, "a 16-byte piece reaches past the range");
                    ++hit[p.head + 2 * q];
                    ++hit[p.head + 2 * q + 1];
                }
                if (p.tail) ++hit[n - 1];
                for (uint64_t w = 0; w < n; ++w) MUST(hit[w] == 1, "word %llu written %d times", (unsigned long long)w, hit[w]);
            }
    MUST(gather_sigma_wide(128, 0x7f00) && !gather_sigma_wide(128, 0x7f08) && !gather_sigma_wide(3, 0) && !gather_sigma_wide(0, 0),
         "the wide sigma rule");
}

int main() {
    std::mt19937_64 rng(20240607);
    for (uint32_t sw : {0u, 3u, 128u}) {
        const gather_geom g = gather_geom_of(sw);
        MUST(g.ept >= 1 && (uint64_t)g.ept * gather_edge_bytes(sw) <= kGatherTileBytes, "ept %u", g.ept);
        MUST((uint64_t)(g.ept + 1) * gather_edge_bytes(sw) > kGatherTileBytes, "ept %u is not the most a tile holds", g.ept);
        MUST(g.lpt >= 1 && (uint64_t)g.lpt * kGatherLayerBytes <= kGatherTileBytes, "lpt %u", g.lpt);
        const std::vector<uint64_t> edgeE = {0, 1, (uint64_t)g.ept - 1, g.ept, (uint64_t)g.ept + 1, 2ull * g.ept + 1};
        const std::vector<uint64_t> edgeL = {0, 1, (uint64_t)g.lpt - 1, g.lpt, (uint64_t)g.lpt + 1, 2ull * g.lpt + 1};
        // every boundary count against every other, alone and in one batch
        for (uint64_t e : edgeE)
            for (uint64_t l : edgeL) check_batch({e}, {l}, sw);
        check_batch(edgeE, edgeL, sw);
        check_batch({}, {}, sw);
        check_batch({0, 0, 0}, {0, 0, 0}, sw);
        for (int round = 0; round < 20; ++round) {
            const size_t n = 1 + rng() % 200;
            std::vector<uint64_t> E(n), L(n);
            for (size_t i = 0; i < n; ++i) {
                const uint64_t r = rng() % 10;
                E[i] = r < 3 ? 0 : r < 5 ? edgeE[rng() % edgeE.size()] : r < 9 ? rng() % 50 : rng() % (3ull * g.ept);
                const uint64_t q = rng() % 10;
                L[i] = q < 3 ? 0 : q < 5 ? edgeL[rng() % edgeL.size()] : q < 9 ? rng() % 12 : rng() % (3ull * g.lpt);
            }
            check_batch(E, L, sw);
        }
    }
    check_split();
    std::printf("gather_tiles_check: ok (%ld checks)\n", g_checks);
    return 0;
}
