// metrics_split.hpp — the work split of pvac_hip_sigma_bytehist (k_metrics.hip): shares per cipher,
// the items of share s, its counting rounds and the grid. Pure integer arithmetic: no HIP runtime
// calls and no other header of the library, so it is checked without a GPU
// (tests/cpp/metrics_split_check.cpp). The kernel calls the same functions, so what the check proves
// is what runs.
//
// Terms. An ITEM is what one thread loads in one loop iteration: a 16-byte unit of the cipher's dense
// sigma range on the wide path (rows of mw = sigma_words words, mw even, base 16-byte aligned), one
// 8-byte word of a row's first mw words on the strided path. A UNIT is what shares are cut from: an
// item on the wide path, a whole row on the strided path (so a share's words are (rows) x mw and a
// row never straddles two shares). Share s of `splits` takes units [lo, hi) = [s per, (s + 1) per)
// clipped to the cipher, per = ceil(units / splits). A share's items are counted in ROUNDS of
// kHistRoundItems: after every round the workgroup folds its LDS counters into 64-bit registers (and
// clears them for the next round), which is what bounds a counter (hist_counter_bound).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PVHIP_SPLIT_FN __host__ __device__ inline
#else
#define PVHIP_SPLIT_FN inline
#endif

namespace pvhip {

constexpr uint32_t kHistBlock = 256;             // threads per workgroup
constexpr uint32_t kHistCopies = 32;             // LDS copies of every bin: the copy index is lane % 32
constexpr uint32_t kHistRoundIters = 4096;       // loop iterations of one thread per round
constexpr uint64_t kHistRoundItems = (uint64_t)kHistBlock * kHistRoundIters;
constexpr uint32_t kHistMaxSplits = 4096;

// shares per cipher: sigma_popcount's policy, enough workgroups for 8 per CU, one share per cipher
// from 8 x CU count ciphers on
PVHIP_SPLIT_FN uint32_t hist_splits(uint64_t n, uint32_t num_cus) {
    if (!n) return 1;
    const uint64_t want = (uint64_t)num_cus * 8;
    uint64_t s = (want + n - 1) / n;
    if (s < 1) s = 1;
    if (s > kHistMaxSplits) s = kHistMaxSplits;
    return (uint32_t)s;
}

// one workgroup per (cipher, share); 0 = beyond a launch's 2^31 - 1 workgroups
PVHIP_SPLIT_FN uint64_t hist_grid(uint64_t n, uint32_t splits) {
    const uint64_t g = n * (uint64_t)splits;
    return g > 0x7FFFFFFFull ? 0 : g;
}

// the wide path's condition
PVHIP_SPLIT_FN bool hist_wide(uint32_t mw, uint32_t sigma_words, uint64_t base_addr) {
    return mw == sigma_words && !(mw & 1u) && (base_addr & 15u) == 0;
}

// units of a cipher of `rows` sigma rows
PVHIP_SPLIT_FN uint64_t hist_units(uint64_t rows, uint32_t mw, bool wide) { return wide ? rows * (mw / 2) : rows; }

// units [lo, hi) of share s
PVHIP_SPLIT_FN void hist_share(uint64_t units, uint32_t splits, uint32_t s, uint64_t& lo, uint64_t& hi) {
    const uint64_t per = (units + splits - 1) / splits;
    lo = (uint64_t)s * per;
    if (lo > units) lo = units;
    hi = lo + per;
    if (hi > units) hi = units;
}

// items of a share of `units` units
PVHIP_SPLIT_FN uint64_t hist_items(uint64_t units, uint32_t mw, bool wide) { return wide ? units : units * mw; }

// rounds of a share of `items` items; round r takes items [r kHistRoundItems, (r + 1) kHistRoundItems)
// of the share, clipped
PVHIP_SPLIT_FN uint64_t hist_rounds(uint64_t items) { return (items + kHistRoundItems - 1) / kHistRoundItems; }

// The largest value an LDS counter can reach. A counter (bin, copy) is incremented by the threads
// whose lane % kHistCopies == copy: kHistBlock / kHistCopies of them. In one round a thread runs at
// most kHistRoundIters iterations (thread t takes items t, t + kHistBlock, ... of the round's
// kHistRoundItems) of 16 bytes (wide) or 8 (strided), and all of them can hit one bin.
PVHIP_SPLIT_FN uint64_t hist_counter_bound(bool wide) {
    return (uint64_t)(kHistBlock / kHistCopies) * kHistRoundIters * (wide ? 16u : 8u);
}
static_assert((uint64_t)(kHistBlock / kHistCopies) * kHistRoundIters * 16u < (1ull << 32),
              "a 32-bit LDS counter cannot wrap within a round");

}  // namespace pvhip
