// fp_fold_gate_check.cpp — the writer's gated canonical finish without a GPU (csrc/fp127.hpp):
// fp_fold3_48_words + (only where fp_fold3_48_rare says so) fp_fold3_48_finish, as k_ct_mul_fresh3's
// writer runs them, against fp_fold3_48 and against the value mod p computed with unsigned __int128.
// The gate must be necessary (a lane it lets pass is canonical and not 0 as it stands) and the gated
// result must equal the ungated one for limb triples that fold to 0, p, p +- 1, 2^127, 2^127 + 1,
// to values whose top word is 0x7FFFFFFF or 0 without being p or 0, at 4,096 maximal addends, and
// for 10^6 random triples inside the bounds (l0, l1 < 2^60, l2 < 2^44). A last block checks the
// fold for any u64 l0, l1 and l2 < 2^52, the bounds a product split as L + 2 H would need.
// A stand-alone host program (tests/test_fp_fold_gate.py builds it with ASan + UBSan); fake_hip.hpp
// gives the HIP types and the CHECK macro, the two device builtins fp127.hpp uses get host stand-ins.
#include "fake_hip.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

#if !__has_builtin(__builtin_amdgcn_alignbit)
static inline uint32_t __builtin_amdgcn_alignbit(uint32_t hi, uint32_t lo, uint32_t sh) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31u));
}
#endif
#if !__has_builtin(__builtin_addc)
static inline unsigned __builtin_addc(unsigned a, unsigned b, unsigned ci, unsigned* co) {
    const uint64_t s = (uint64_t)a + b + ci;
    *co = (unsigned)(s >> 32);
    return (unsigned)s;
}
#endif
#include "fp127.hpp"

using namespace pvhip;
typedef unsigned __int128 u128;

static const u128 kP = ((u128)1 << 127) - 1;
static long g_checks = 0, g_gated = 0, g_zero = 0;

static u128 mk(uint64_t lo, uint64_t hi) { return ((u128)hi << 64) | lo; }

static uint64_t g_rng = 0x243F6A8885A308D3ull;   // splitmix64, seeded
static uint64_t rnd() {
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// (l0 + l1 2^48 + l2 2^96) mod p for any u64 l0, l1 and l2 < 2^52; 2^127 == 1 (mod p)
static u128 value_mod_p(uint64_t l0, uint64_t l1, uint64_t l2) {
    u128 s = (u128)l0 % kP;
    s = (s + (((u128)l1 << 48) % kP)) % kP;                       // < 2^112
    s = (s + (((u128)(l2 & 0x7FFFFFFFull) << 96) % kP)) % kP;     // low 31 bits of l2: < 2^127
    s = (s + (u128)(l2 >> 31)) % kP;                              // (l2 >> 31) 2^127 == l2 >> 31
    return s;
}

// the writer's sequence: the fold, the gate, the finish only inside the gate
static fp gated(uint64_t l0, uint64_t l1, uint64_t l2, bool& rare) {
    uint32_t x[4];
    fp_fold3_48_words(l0, l1, l2, x);
    rare = fp_fold3_48_rare(x);
    if (rare) return fp_fold3_48_finish(x);
    return fp{join32(x[0], x[1]), join32(x[2], x[3])};
}

static void check_triple(uint64_t l0, uint64_t l1, uint64_t l2, const char* what) {
    bool rare;
    const fp g = gated(l0, l1, l2, rare);
    const fp f = fp_fold3_48(l0, l1, l2);
    const u128 want = value_mod_p(l0, l1, l2);
    CHECK(g.lo == f.lo && g.hi == f.hi, "%s: gated %016llx%016llx, fp_fold3_48 %016llx%016llx (limbs %llx %llx %llx)", what,
          (unsigned long long)g.hi, (unsigned long long)g.lo, (unsigned long long)f.hi, (unsigned long long)f.lo,
          (unsigned long long)l0, (unsigned long long)l1, (unsigned long long)l2);
    CHECK(mk(g.lo, g.hi) == want, "%s: gated fold is not the value mod p (limbs %llx %llx %llx)", what, (unsigned long long)l0,
          (unsigned long long)l1, (unsigned long long)l2);
    // necessary: a 0 is only ever produced inside the gate
    CHECK(rare || (g.lo | g.hi) != 0, "%s: a zero outside the gate", what);
    g_gated += rare;
    g_zero += (g.lo | g.hi) == 0;
    ++g_checks;
}

// Limb triples with l0 + l1 2^48 + l2 2^96 == v + k p for the k given: the plain cut of the sum
// and cuts that move up to 2^12 - 1 units down from limb 1 into limb 0 and from limb 2 into limb 1
// (what 4,096 addends can pile up), all inside l0, l1 < 2^60, l2 < 2^44.
static void check_value(u128 v, const char* what) {
    for (uint64_t k : {0ull, 1ull, 2ull, 3ull, 1599ull, 4095ull, 8190ull}) {
        // v + k p < 2^128 + 2^140 does not fit: carry the sum as (low 96 bits, rest)
        const u128 m96 = ((u128)1 << 96) - 1;
        u128 low = (v & m96), high = v >> 96;                  // v = high 2^96 + low
        // k p = k 2^127 - k = (k 2^31) 2^96 - k
        high += (u128)k << 31;
        if (low >= k) low -= k; else { low = low + ((u128)1 << 96) - k; CHECK(high > 0, "borrow"); high -= 1; }
        const uint64_t c0 = (uint64_t)(low & 0xFFFFFFFFFFFFull), c1 = (uint64_t)(low >> 48), c2 = (uint64_t)high;
        if (c2 >= (1ull << 44)) continue;                      // past the bound of limb 2
        check_triple(c0, c1, c2, what);
        for (uint64_t a : {1ull, 2ull, 4095ull})
            for (uint64_t b : {0ull, 1ull, 4095ull}) {
                if (c1 < a || c2 < b) continue;
                const uint64_t m0 = c0 + (a << 48), m1 = c1 - a + (b << 48), m2 = c2 - b;
                if (m0 < (1ull << 60) && m1 < (1ull << 60)) check_triple(m0, m1, m2, what);
            }
    }
}

int main() {
    const u128 one = 1;
    // the values the gate is about
    check_value(0, "0");
    check_value(kP, "p");
    check_value(kP - 1, "p - 1");
    check_value(kP + 1, "p + 1");
    check_value(one << 127, "2^127");
    check_value((one << 127) + 1, "2^127 + 1");
    check_value(1, "1");
    // top word 0x7FFFFFFF without being p: every single cleared bit below it, random low words
    for (int b = 0; b < 96; ++b) check_value(kP - (one << b), "x3 == 0x7FFFFFFF, not p");
    for (int k = 0; k < 2000; ++k) {
        const uint64_t lo = rnd();
        check_value(((u128)0x7FFFFFFFull << 96) | ((u128)(rnd() & 0xFFFFFFFFull) << 64) | lo, "x3 == 0x7FFFFFFF, not p");
    }
    // top word 0 without being 0: every single bit below bit 96, random values below 2^96
    for (int b = 0; b < 96; ++b) check_value(one << b, "x3 == 0, not 0");
    for (int k = 0; k < 2000; ++k) {
        const uint64_t lo = rnd();
        check_value(((u128)(rnd() & 0xFFFFFFFFull) << 64) | lo, "x3 == 0, not 0");
    }
    const long zeros_wanted = g_zero;
    CHECK(zeros_wanted > 0, "no triple folded to 0");

    // capacity: 4,096 maximal addends of the 48/48/32-bit cuts, and one unit less in each limb
    {
        const uint64_t n = kLimb48MaxAddends;
        const uint64_t L0 = n * ((1ull << 48) - 1), L1 = n * ((1ull << 48) - 1), L2 = n * ((1ull << 32) - 1);
        CHECK(L0 < (1ull << 60) && L1 < (1ull << 60) && L2 < (1ull << 44), "capacity bounds");
        for (uint64_t d0 : {0ull, 1ull})
            for (uint64_t d1 : {0ull, 1ull})
                for (uint64_t d2 : {0ull, 1ull}) check_triple(L0 - d0, L1 - d1, L2 - d2, "4096 maximal addends");
        check_triple((1ull << 60) - 1, (1ull << 60) - 1, (1ull << 44) - 1, "every limb at its bound");
    }

    // 10^6 random triples inside the bounds; of uniform triples the gate passes all but a few
    const long gated_before = g_gated;
    for (int k = 0; k < 1000000; ++k) check_triple(rnd() >> 4, rnd() >> 4, rnd() >> 20, "random");
    CHECK(g_gated - gated_before < 100, "the gate fired for %ld of 10^6 uniform triples", g_gated - gated_before);

    // the fold itself for any u64 l0, l1 and l2 < 2^52 (x < 2^127 + 2^22 before the last step)
    for (uint64_t l0 : {0ull, 1ull, ~0ull})
        for (uint64_t l1 : {0ull, 1ull, ~0ull})
            for (uint64_t l2 : {0ull, 1ull, (1ull << 52) - 1, 0x7FFFFFFFull, 0x80000000ull}) check_triple(l0, l1, l2, "wide corners");
    for (int k = 0; k < 200000; ++k) check_triple(rnd(), rnd(), rnd() >> 12, "wide random");

    if (g_fail) {
        std::fprintf(stderr, "fp_fold_gate_check: %d failure(s)\n", g_fail);
        return 1;
    }
    std::printf("fp_fold_gate_check: ok (%ld checks, %ld gated, %ld zeros)\n", g_checks, g_gated, g_zero);
    return 0;
}
