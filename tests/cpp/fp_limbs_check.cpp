// fp_limbs_check.cpp — the fresh ct_mul kernel's limb accumulators without a GPU (csrc/fp127.hpp):
// fp_split3_48 / fp_fold3_48 (48/48/32-bit limbs on byte-aligned cuts) against the sum mod p computed
// with unsigned __int128 and against the 44/44/40 pair they replace in k_ct_mul_fresh3, at 1, 2, 3,
// 4095 and 4096 addends; the cell id in bits 52..63 of limb 2 under 4,096 maximal addends; and
// fp_mul_fold1f (first row word through the multiply's addend) against fp_mul_fold1.
// A stand-alone host program (tests/test_fp_limbs.py builds it with ASan + UBSan); fake_hip.hpp gives
// the HIP types and the CHECK macro, the two device builtins fp127.hpp uses get host stand-ins here.
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
static long g_checks = 0;

static u128 mk(uint64_t lo, uint64_t hi) { return ((u128)hi << 64) | lo; }
static uint64_t lo64(u128 x) { return (uint64_t)x; }
static uint64_t hi64(u128 x) { return (uint64_t)(x >> 64); }

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;   // splitmix64, seeded
static uint64_t rnd() {
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the boundary values: 0, 1, p - 1 = 2^127 - 2, p, 2^128 - 1, every value with a single 16-bit word
// all ones, and every run of 2..4 set bits across the cuts 47/48 and 95/96 (alone and on both cuts)
static std::vector<u128> boundary_values() {
    std::vector<u128> v = {0, 1, kP - 1, ((u128)1 << 127) - 2, kP, ~(u128)0, (u128)1 << 127};
    for (int w = 0; w < 8; ++w) v.push_back((u128)0xFFFFu << (16 * w));
    std::vector<u128> c47, c95;
    for (int lo = 1; lo <= 2; ++lo)
        for (int hi = 1; hi <= 2; ++hi) {
            const u128 run = ((u128)1 << (lo + hi)) - 1;
            c47.push_back(run << (48 - lo));
            c95.push_back(run << (96 - lo));
        }
    for (u128 a : c47) v.push_back(a);
    for (u128 b : c95) v.push_back(b);
    for (u128 a : c47)
        for (u128 b : c95) v.push_back(a | b);
    v.push_back(((u128)1 << 48) - 1);    // all of limb 0
    v.push_back(((u128)1 << 96) - 1);    // all of limbs 0 and 1
    v.push_back(~(((u128)1 << 96) - 1)); // all of limb 2
    return v;
}

// N addends starting at vals[at] (cyclic): the fold of the summed limbs against the sum mod p and
// against the 44/44/40 pair
static void check_window(const std::vector<u128>& vals, size_t at, int n, const char* what) {
    uint64_t s48[3] = {0, 0, 0}, s44[3] = {0, 0, 0};
    u128 want = 0;
    for (int k = 0; k < n; ++k) {
        const u128 x = vals[(at + (size_t)k) % vals.size()];
        uint64_t l0, l1, l2;
        fp_split3_48(lo64(x), hi64(x), l0, l1, l2);
        CHECK(l0 < (1ull << 48) && l1 < (1ull << 48) && l2 < (1ull << 32), "%s: a 48/48/32 limb too wide", what);
        CHECK((u128)l0 + ((u128)l1 << 48) + ((u128)l2 << 96) == x, "%s: the limbs do not give x back", what);
        s48[0] += l0; s48[1] += l1; s48[2] += l2;
        fp_split3_44(lo64(x), hi64(x), l0, l1, l2);
        s44[0] += l0; s44[1] += l1; s44[2] += l2;
        want = (want + x % kP) % kP;   // both below 2^127: no overflow
    }
    CHECK(s48[0] < (1ull << 60) && s48[1] < (1ull << 60) && s48[2] < (1ull << 44), "%s: limb sums past their bounds", what);
    const fp a = fp_fold3_48(s48[0], s48[1], s48[2]);
    const fp b = fp_fold3_44(s44[0], s44[1], s44[2]);
    CHECK(mk(a.lo, a.hi) == want, "%s: %d addends at %zu: fold3_48 %016llx%016llx, sum mod p %016llx%016llx", what, n, at,
          (unsigned long long)a.hi, (unsigned long long)a.lo, (unsigned long long)hi64(want), (unsigned long long)lo64(want));
    CHECK(a.lo == b.lo && a.hi == b.hi, "%s: %d addends at %zu: fold3_48 differs from fold3_44", what, n, at);
    ++g_checks;
}

static void check_mul(u128 x, u128 y) {
    const fp a = fp_canon(lo64(x), hi64(x)), b = fp_canon(lo64(y), hi64(y));   // the kernel stages canonical weights
    uint64_t o0, o1, n0, n1;
    fp_mul_fold1(a, b, o0, o1);
    fp_mul_fold1f(a, b, n0, n1);
    CHECK(o0 == n0 && o1 == n1, "fp_mul_fold1f differs from fp_mul_fold1 for %016llx%016llx * %016llx%016llx",
          (unsigned long long)a.hi, (unsigned long long)a.lo, (unsigned long long)b.hi, (unsigned long long)b.lo);
    ++g_checks;
}

int main() {
    const std::vector<u128> bnd = boundary_values();
    std::vector<u128> rnds(100000);
    for (u128& x : rnds) {
        const uint64_t lo = rnd();
        x = mk(lo, rnd());
    }
    std::vector<u128> all = bnd;
    all.insert(all.end(), rnds.begin(), rnds.end());

    // 1, 2, 3 addends: every window of the whole value set (boundary values first, so they also
    // meet each other and the first random values)
    for (int n = 1; n <= 3; ++n)
        for (size_t at = 0; at < all.size(); ++at) check_window(all, at, n, "small");
    // 4095 and 4096 addends: one value repeated (every boundary value, so 4,096 times 2^128 - 1 too),
    // the boundary set cycled from every start, and windows through the random values
    for (int n : {4095, 4096}) {
        for (u128 x : bnd) check_window(std::vector<u128>{x}, 0, n, "repeated");
        for (size_t at = 0; at < bnd.size(); ++at) check_window(bnd, at, n, "boundary cycle");
        for (size_t at = 0; at + (size_t)n <= rnds.size(); at += 4099) check_window(rnds, at, n, "random");
    }
    // capacity, the kernel's bound: the cell id at bits 52..63 of limb 2 under 4,096 maximal addends
    for (uint64_t cell : {0ull, 1ull, 0x555ull, 0xAAAull, 0xFFFull}) {
        uint64_t s[3] = {0, 0, cell << 52};
        for (uint32_t k = 0; k < kLimb48MaxAddends; ++k) {
            uint64_t l0, l1, l2;
            fp_split3_48(~0ull, ~0ull, l0, l1, l2);
            s[0] += l0; s[1] += l1; s[2] += l2;
        }
        CHECK(s[2] >> 52 == cell, "cell id %llx became %llx", (unsigned long long)cell, (unsigned long long)(s[2] >> 52));
        CHECK(s[0] < (1ull << 60) && s[1] < (1ull << 60), "limbs 0 / 1 reached 2^60");
        const fp w = fp_fold3_48(s[0], s[1], s[2] & ((1ull << 52) - 1ull));
        const u128 want = (((~(u128)0) % kP) * kLimb48MaxAddends) % kP;   // 1 * 4096
        CHECK(mk(w.lo, w.hi) == want, "4096 maximal addends under cell %llx", (unsigned long long)cell);
        ++g_checks;
    }
    // fp_mul_fold1f against fp_mul_fold1: the boundary set crossed with itself, with 1,000 random
    // values on either side, and 10^5 random pairs
    for (u128 x : bnd)
        for (u128 y : bnd) check_mul(x, y);
    for (u128 x : bnd)
        for (size_t k = 0; k < 1000; ++k) {
            check_mul(x, rnds[k]);
            check_mul(rnds[k], x);
        }
    for (size_t k = 0; k < rnds.size(); ++k) check_mul(rnds[k], rnds[(k + 1) % rnds.size()]);

    if (g_fail) {
        std::fprintf(stderr, "fp_limbs_check: %d failure(s)\n", g_fail);
        return 1;
    }
    std::printf("fp_limbs_check: ok (%ld checks)\n", g_checks);
    return 0;
}
