// metrics_split_check.cpp — csrc/metrics_split.hpp without a GPU: the shares of a cipher tile its units
// exactly once and in order, a share's rounds tile its items, the grid stays within a launch's 2^31 - 1
// workgroups, and the per-counter bound the kernel comment states holds for the largest share. Built
// stand-alone with ASan + UBSan by tests/test_metrics_split.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "metrics_split.hpp"

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

// one cipher of `rows` rows under `splits` shares: returns the most items a share holds
static uint64_t check_cipher(uint64_t rows, uint32_t mw, bool wide, uint32_t splits) {
    const uint64_t units = hist_units(rows, mw, wide);
    MUST(units == (wide ? rows * (mw / 2) : rows), "units");
    uint64_t next = 0, max_items = 0, bytes = 0;
    for (uint32_t s = 0; s < splits; ++s) {
        uint64_t lo, hi;
        hist_share(units, splits, s, lo, hi);
        MUST(lo <= hi && hi <= units, "share %u of %u: [%llu, %llu) of %llu", s, splits, (unsigned long long)lo,
             (unsigned long long)hi, (unsigned long long)units);
        MUST(lo == next, "share %u of %u starts at %llu, expected %llu", s, splits, (unsigned long long)lo,
             (unsigned long long)next);
        next = hi;
        const uint64_t items = hist_items(hi - lo, mw, wide);
        bytes += items * (wide ? 16 : 8);
        if (items > max_items) max_items = items;
        // rounds tile the share's items in order, each within kHistRoundItems
        const uint64_t rounds = hist_rounds(items);
        MUST((items == 0) == (rounds == 0), "rounds of an empty share");
        if (rounds) {
            MUST((rounds - 1) * kHistRoundItems < items && items <= rounds * kHistRoundItems, "rounds of %llu items",
                 (unsigned long long)items);
            // thread t's iterations in a full round: t, t + kHistBlock, ... below kHistRoundItems
            MUST((kHistRoundItems + kHistBlock - 1) / kHistBlock == kHistRoundIters, "iterations per round");
        }
    }
    MUST(next == units, "the shares end at %llu of %llu units", (unsigned long long)next, (unsigned long long)units);
    MUST(bytes == rows * mw * 8, "the shares hold %llu bytes of %llu", (unsigned long long)bytes,
         (unsigned long long)(rows * mw * 8));
    return max_items;
}

int main() {
    const uint64_t ns[] = {1, 2, 2047, 2048, 1ull << 20, 0x7FFFFFFFull};
    const uint64_t rows[] = {0, 1, 40, 513, 1ull << 23};
    const uint32_t cus[] = {1, 64, 256, 304};
    struct { uint32_t mw, sw; uint64_t addr; bool wide; } paths[] = {
        {128, 128, 0x1000, true}, {128, 128, 0x1008, false}, {5, 5, 0x1000, false}, {4, 6, 0x1000, false}, {2, 2, 0x10, true}};
    for (auto& pt : paths) MUST(hist_wide(pt.mw, pt.sw, pt.addr) == pt.wide, "path of mw %u sw %u", pt.mw, pt.sw);

    uint64_t largest = 0;
    for (uint32_t cu : cus)
        for (uint64_t n : ns) {
            const uint32_t splits = hist_splits(n, cu);
            MUST(splits >= 1 && splits <= kHistMaxSplits, "splits %u", splits);
            MUST(n < 8ull * cu || splits == 1, "from 8 x CU count ciphers on a cipher has one share (n %llu, %u CUs: %u)",
                 (unsigned long long)n, cu, splits);
            const uint64_t grid = hist_grid(n, splits);
            MUST(grid == n * splits && grid >= 1 && grid <= 0x7FFFFFFFull, "grid of n %llu x %u", (unsigned long long)n, splits);
            for (auto& pt : paths)
                for (uint64_t r : rows) {
                    const uint64_t m = check_cipher(r, pt.mw, pt.wide, splits);
                    if (m > largest) largest = m;
                }
        }
    MUST(hist_grid(0x80000000ull, 1) == 0 && hist_grid(0x7FFFFFFFull, 2) == 0, "a grid beyond 2^31 - 1 is refused");
    MUST(hist_splits(0, 256) == 1, "n = 0");

    // the bound: the largest share here (one workgroup owning 2^23 rows of 1 KiB) is far longer than a
    // round, and a counter still sees at most 8 threads x 4096 items x 16 bytes between two folds
    MUST(largest == (1ull << 23) * 128 && largest > kHistRoundItems, "largest share: %llu items", (unsigned long long)largest);
    for (int wide = 0; wide < 2; ++wide) {
        const uint64_t per_thread = (kHistRoundItems + kHistBlock - 1) / kHistBlock;   // items of one thread per round
        const uint64_t bound = (uint64_t)(kHistBlock / kHistCopies) * per_thread * (wide ? 16 : 8);
        MUST(bound == hist_counter_bound(wide != 0), "counter bound (wide %d)", wide);
        MUST(bound < (1ull << 32), "a u32 counter wraps at %llu", (unsigned long long)bound);
    }
    MUST(hist_counter_bound(true) == (1ull << 19), "the bound the kernel comment states");
    MUST(kHistBlock % kHistCopies == 0 && kHistCopies == 32, "one copy per bank of a 32-lane group");
    std::printf("metrics_split_check: ok (%ld checks)\n", g_checks);
    return 0;
}
