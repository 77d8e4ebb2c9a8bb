// large_plan_check.cpp — csrc/large_plan.hpp without a GPU: a general-path pair's scratch layout
// (build_large_desc, rebase_desc), the shared-bucket test and the cut of a pair set into sub-batches
// (cut_sub_batch). Host code only; built with ASan + UBSan by tests/test_large_plan.py.
//
// The expected values in the tables below were printed by the code as it stood BEFORE it moved into
// large_plan.hpp (build_large_desc and rebase_desc in the host runtime, the sub-batch loop inside
// run_large, now in csrc/rt_mul.cpp): the move must not change one of them. A change that is meant to change a layout or a
// launch size has to justify the new numbers and replace the rows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "large_plan.hpp"

using namespace pvhip;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            ++g_failed;                                                              \
        }                                                                            \
    } while (0)

// (LA, LB, nA, nB, Bm, static_grp, allow_direct)
struct shape {
    uint64_t LA, LB, nA, nB;
    uint32_t Bm;
    bool sg, ad;
};
const shape kShapes[] = {
    {1, 1, 1, 1, 337, false, false},              //  0 the minimum, four ways
    {1, 1, 1, 1, 337, false, true},               //  1
    {1, 1, 1, 1, 337, true, false},               //  2
    {1, 1, 1, 1, 337, true, true},                //  3
    {8, 1, 320, 20, 337, true, true},             //  4 a chain step-2 pair: direct
    {8, 1, 320, 20, 337, true, false},            //  5 ... and iblk on the full layout
    {2, 2, 96, 63, 337, true, true},              //  6 iblk stops at |B.E| = 64
    {2, 2, 96, 64, 337, true, true},              //  7
    {4, 4, 200, 40, 337, true, true},             //  8 kLaMaxLB: o_defer only at LB <= 4
    {4, 5, 200, 40, 337, true, true},             //  9
    {1, 1, (1u << 21) - 1, 1, 337, true, true},   // 10 direct's 21-bit edge id
    {1, 1, 1u << 21, 1, 337, true, true},         // 11
    {2, 1, 96, 20, 1024, true, true},             // 12 direct's B <= 1024
    {2, 1, 96, 20, 1025, true, true},             // 13
    {2, 12, 96, 20, 337, true, true},             // 14 dir_lds_bytes(337, 13) is the first above 160 KiB
    {2, 13, 96, 20, 337, true, true},             // 15 (LB > kLaMaxLB is never direct anyway)
    {2, 3, 96, 20, 1024, true, true},             // 16 where the LDS bound decides: B = 1024, LB = 3 fits,
    {2, 4, 96, 20, 1024, true, true},             // 17 LB = 4 does not
    {1, 1, 0, 1, 337, true, true},                // 18 no A edges: n = 0, capE = 0
    {1, 1, 0, 1, 337, false, false},              // 19
    {3, 6, 50, 70, 337, false, false},            // 20 dynamic chains, per-task products
    {2, 2, 96, 63, 337, true, false},             // 21 iblk, not direct
    {9, 2, 500, 30, 337, true, false},            // 22 iblk, two A-layer workgroups
    {2, 1, 96, 20, 337, true, true},              // 23 direct
    {1, 1, 65536, 65536, 337, false, false},      // 24 refused: n = 2^32
    {1, 8192, 10, 10, 337, false, false},         // 25 refused: Lc = kLargeLayersMax + 1
    {64, 128, 10, 10, 1u << 18, false, false},    // 26 refused: S = 2^31
};
constexpr size_t kNumShapes = sizeof kShapes / sizeof kShapes[0];
constexpr size_t kNumAccepted = 24;

// every field of large_desc, in declaration order
constexpr int kF = 48;
const char* const kFieldNames[kF] = {
    "pair", "n", "S", "Lc", "nblk", "capE", "nbm.d", "nbm.m", "LA", "LB", "nA", "nB", "hbits", "iblk", "direct", "pad_d",
    "nb_m", "g_head", "g_next", "o_zero", "zero_words", "o_cnt", "o_hkey", "o_hhead", "o_bmask", "o_bcnt", "o_used",
    "o_tkey", "o_lstA", "o_lstB", "o_neA", "o_neB", "o_defer", "o_info", "o_sums", "o_nxt", "o_tb", "o_within", "o_etot",
    "o_cpos", "o_order", "o_hpos", "o_icnt", "o_imask", "o_wle", "o_wln", "o_iwo", "words"};
constexpr int kFirstOffset = 19;   // o_zero; zero_words (20) and words (47) are sizes
void fields(const large_desc& d, uint64_t* f) {
    const uint64_t v[kF] = {d.pair, d.n, d.S, d.Lc, d.nblk, d.capE, d.nbm.d, d.nbm.m, d.LA, d.LB, d.nA, d.nB, d.hbits, d.iblk,
                            d.direct, d.pad_d, d.nb_m, d.g_head, d.g_next, d.o_zero, d.zero_words, d.o_cnt, d.o_hkey,
                            d.o_hhead, d.o_bmask, d.o_bcnt, d.o_used, d.o_tkey, d.o_lstA, d.o_lstB, d.o_neA, d.o_neB,
                            d.o_defer, d.o_info, d.o_sums, d.o_nxt, d.o_tb, d.o_within, d.o_etot, d.o_cpos, d.o_order,
                            d.o_hpos, d.o_icnt, d.o_imask, d.o_wle, d.o_wln, d.o_iwo, d.words};
    std::memcpy(f, v, sizeof v);
}
static_assert(sizeof(large_desc) == 40 * 8 + 8 * 4, "large_desc changed: add the field to fields() and the tables");

// shape s built with pair id 7 + s: rc, then the fields
const uint64_t kDescExp[kNumAccepted][1 + kF] = {
    /*  0 */ {0, 7, 1, 337, 3, 1, 2, 2, 0x7fffffffffffffffull, 1, 1, 1, 1, 1, 0, 0, 0, 0x100000000ull, kNoGrp, kNoGrp, 0, 27, 0, 16, 20, 22, 24, 24, 27, 364, 367, 370, 371, 372, 373, 712, 3408, 3745, 4082, 4419, 4756, 5093, 5095, 5097, 5100, 5100, 5100, 5100, 5100},
    /*  1 */ {0, 8, 1, 337, 3, 1, 2, 2, 0x7fffffffffffffffull, 1, 1, 1, 1, 1, 0, 0, 0, 0x100000000ull, kNoGrp, kNoGrp, 0, 27, 0, 16, 20, 22, 24, 24, 27, 364, 367, 370, 371, 372, 373, 712, 3408, 3745, 4082, 4419, 4756, 5093, 5095, 5097, 5100, 5100, 5100, 5100, 5100},
    /*  2 */ {0, 9, 1, 337, 3, 1, 2, 2, 0x7fffffffffffffffull, 1, 1, 1, 1, 1, 1, 0, 0, 0x100000000ull, kNoGrp, kNoGrp, 0, 21, 0, 16, 16, 16, 18, 18, 21, 358, 361, 364, 365, 366, 367, 704, 3400, 3400, 3737, 4074, 4411, 4748, 4750, 4752, 4756, 4760, 4760, 4760, 4760},
    /*  3 */ {0, 10, 1, 337, 3, 1, 2, 2, 0x7fffffffffffffffull, 1, 1, 1, 1, 1, 1, 1, 0, 0x100000000ull, kNoGrp, kNoGrp, 0, 19, 0, 16, 16, 16, 16, 16, 19, 19, 22, 25, 26, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 28, 40, 37, 38, 36, 44},
    /*  4 */ {0, 11, 6400, 2696, 17, 400, 5392, 6427, 0xa326d60e94186ull, 8, 1, 320, 20, 13, 1, 1, 0, 214748364, kNoGrp, kNoGrp, 0, 33, 0, 16, 16, 16, 16, 16, 33, 33, 369, 391, 399, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 820, 490, 810, 480, 2100},
    /*  5 */ {0, 12, 6400, 2696, 17, 400, 5392, 6427, 0xa326d60e94186ull, 8, 1, 320, 20, 13, 1, 0, 0, 214748364, kNoGrp, kNoGrp, 0, 833, 0, 16, 16, 16, 816, 816, 833, 3529, 3865, 3887, 3895, 3896, 3904, 6600, 28168, 28168, 30864, 33560, 36256, 38952, 44344, 49736, 50056, 51336, 51336, 51336, 51336},
    /*  6 */ {0, 13, 6048, 1348, 8, 378, 2696, 6427, 0xa326d60e94186ull, 2, 2, 96, 63, 12, 1, 1, 0, 68174084, kNoGrp, kNoGrp, 0, 24, 0, 16, 16, 16, 16, 16, 24, 24, 124, 191, 193, 195, 195, 195, 195, 195, 195, 195, 195, 195, 195, 196, 324, 223, 319, 220, 708},
    /*  7 */ {0, 14, 6144, 1348, 8, 384, 2696, 6427, 0xa326d60e94186ull, 2, 2, 96, 64, 12, 0, 0, 0, 67108864, kNoGrp, kNoGrp, 0, 792, 0, 16, 16, 16, 784, 784, 792, 2140, 2240, 2308, 2310, 2312, 2316, 3664, 14448, 14448, 15796, 17144, 18492, 19840, 22536, 25232, 25232, 25232, 25232, 25232, 25232},
    /*  8 */ {0, 15, 8000, 5392, 24, 500, 10784, 8123, 0x8116582e237c8ull, 4, 4, 200, 40, 14, 1, 1, 0, 107374182, kNoGrp, kNoGrp, 0, 40, 0, 16, 16, 16, 16, 16, 40, 40, 248, 296, 300, 304, 304, 304, 304, 304, 304, 304, 304, 304, 304, 304, 572, 367, 567, 360, 1372},
    /*  9 */ {0, 16, 8000, 6740, 29, 500, 13480, 8123, 0x8116582e237c8ull, 4, 5, 200, 40, 14, 0, 0, 0, 107374182, kNoGrp, kNoGrp, 0, 1045, 0, 16, 16, 16, 1016, 1016, 1045, 7785, 7993, 8043, 8047, 8052, 8052, 14792, 68712, 68712, 75452, 82192, 88932, 95672, 109152, 122632, 122632, 122632, 122632, 122632, 122632},
    /* 10 */ {0, 17, 2097151, 337, 3, 131072, 674, 2144977, 0x7d256547155ull, 1, 1, 2097151, 1, 10, 1, 1, 0, 0x100000000ull, kNoGrp, kNoGrp, 0, 19, 0, 16, 16, 16, 16, 16, 19, 19, 2097172, 2097175, 2097176, 2097177, 2097177, 2097177, 2097177, 2097177, 2097177, 2097177, 2097177, 2097177, 2097177, 2097180, 4784156, 2687004, 4784155, 2621468, 13172760},
    /* 11 */ {0, 18, 2097152, 337, 3, 131072, 674, 2144977, 0x7d256547155ull, 1, 1, 2097152, 1, 10, 1, 0, 0, 0x100000000ull, kNoGrp, kNoGrp, 0, 262163, 0, 16, 16, 16, 262160, 262160, 262163, 262500, 2359654, 2359657, 2359658, 2359659, 2359660, 2360000, 2362696, 2362696, 2363033, 2363370, 2363707, 2364044, 2364718, 2365392, 4462544, 12851152, 12851152, 12851152, 12851152},
    /* 12 */ {0, 19, 1920, 2048, 5, 120, 3840, 2029, 0x204cb630b3aab5ull, 2, 1, 96, 20, 12, 1, 1, 0, 214748364, kNoGrp, kNoGrp, 0, 21, 0, 16, 16, 16, 16, 16, 21, 21, 121, 143, 145, 146, 146, 146, 146, 146, 146, 146, 146, 146, 146, 148, 276, 175, 271, 172, 660},
    /* 13 */ {0, 20, 1920, 2050, 5, 120, 3840, 2029, 0x204cb630b3aab5ull, 2, 1, 96, 20, 12, 1, 0, 0, 214748364, kNoGrp, kNoGrp, 0, 261, 0, 16, 16, 16, 256, 256, 261, 2311, 2411, 2433, 2435, 2436, 2438, 4488, 20888, 20888, 22938, 24988, 27038, 29088, 32928, 36768, 36864, 37248, 37248, 37248, 37248},
    /* 14 */ {0, 21, 1920, 8088, 38, 120, 3840, 2029, 0x204cb630b3aab5ull, 2, 12, 96, 20, 12, 0, 0, 0, 214748364, kNoGrp, kNoGrp, 0, 294, 0, 16, 16, 16, 256, 256, 294, 8382, 8482, 8526, 8528, 8540, 8540, 16628, 81332, 81332, 89420, 97508, 105596, 113684, 117524, 121364, 121364, 121364, 121364, 121364, 121364},
    /* 15 */ {0, 22, 1920, 8762, 41, 120, 3840, 2029, 0x204cb630b3aab5ull, 2, 13, 96, 20, 12, 0, 0, 0, 214748364, kNoGrp, kNoGrp, 0, 297, 0, 16, 16, 16, 256, 256, 297, 9059, 9159, 9205, 9207, 9220, 9220, 17984, 88080, 88080, 96842, 105604, 114366, 123128, 126968, 130808, 130808, 130808, 130808, 130808, 130808},
    /* 16 */ {0, 23, 1920, 6144, 11, 120, 3840, 2029, 0x204cb630b3aab5ull, 2, 3, 96, 20, 12, 1, 1, 0, 214748364, kNoGrp, kNoGrp, 0, 27, 0, 16, 16, 16, 16, 16, 27, 27, 127, 153, 155, 158, 158, 158, 158, 158, 158, 158, 158, 158, 158, 160, 288, 187, 283, 184, 672},
    /* 17 */ {0, 24, 1920, 8192, 14, 120, 3840, 2029, 0x204cb630b3aab5ull, 2, 4, 96, 20, 12, 1, 0, 0, 214748364, kNoGrp, kNoGrp, 0, 270, 0, 16, 16, 16, 256, 256, 270, 8462, 8562, 8590, 8592, 8596, 8604, 16796, 82332, 82332, 90524, 98716, 106908, 115100, 118940, 122780, 122876, 123260, 123260, 123260, 123260},
    /* 18 */ {0, 25, 0, 337, 3, 0, 0, 2, 0x7fffffffffffffffull, 1, 1, 0, 1, 1, 0, 0, 0, 0x100000000ull, kNoGrp, kNoGrp, 0, 19, 0, 16, 16, 16, 16, 16, 19, 356, 358, 361, 362, 363, 364, 704, 3400, 3400, 3737, 4074, 4411, 4748, 4748, 4748, 4748, 4748, 4748, 4748, 4748},
    /* 19 */ {0, 26, 0, 337, 3, 0, 0, 2, 0x7fffffffffffffffull, 1, 1, 0, 1, 1, 0, 0, 0, 0x100000000ull, kNoGrp, kNoGrp, 0, 25, 0, 16, 20, 22, 22, 22, 25, 362, 364, 367, 368, 369, 370, 708, 3404, 3741, 4078, 4415, 4752, 5089, 5089, 5089, 5092, 5092, 5092, 5092, 5092},
    /* 20 */ {0, 27, 3500, 6066, 27, 219, 7000, 3739, 0x1187161d70e725ull, 3, 6, 50, 70, 13, 0, 0, 0, 61356675, kNoGrp, kNoGrp, 0, 25057, 0, 16, 16400, 24592, 25030, 25030, 25057, 31123, 31179, 31261, 31264, 31270, 31270, 37336, 85864, 91930, 97996, 104062, 110128, 116194, 123194, 130194, 130196, 130196, 130196, 130196, 130196},
    /* 21 */ {0, 28, 6048, 1348, 8, 378, 2696, 6427, 0xa326d60e94186ull, 2, 2, 96, 63, 12, 1, 0, 0, 68174084, kNoGrp, kNoGrp, 0, 780, 0, 16, 16, 16, 772, 772, 780, 2128, 2228, 2295, 2297, 2299, 2303, 3652, 14436, 14436, 15784, 17132, 18480, 19828, 22524, 25220, 25316, 25700, 25700, 25700, 25700},
    /* 22 */ {0, 29, 15000, 6066, 29, 938, 12132, 15173, 0x451ba740bcf79ull, 9, 2, 500, 30, 14, 1, 0, 0, 143165576, kNoGrp, kNoGrp, 0, 1921, 0, 16, 16, 16, 1892, 1892, 1921, 7987, 8505, 8539, 8548, 8550, 8568, 14636, 63164, 63164, 69230, 75296, 81362, 87428, 99560, 111692, 112192, 114192, 114192, 114192, 114192},
    /* 23 */ {0, 30, 1920, 674, 5, 120, 1348, 2029, 0x204cb630b3aab5ull, 2, 1, 96, 20, 11, 1, 1, 0, 214748364, kNoGrp, kNoGrp, 0, 21, 0, 16, 16, 16, 16, 16, 21, 21, 121, 143, 145, 146, 146, 146, 146, 146, 146, 146, 146, 146, 146, 148, 276, 175, 271, 172, 660},
};

// ---------------------------------------------------------------- descriptors
struct span {
    const char* name;
    uint64_t off, len, align;
};

// the arrays of a pair's scratch with the sizes common.hpp documents at large_desc
std::vector<span> arrays_of(const large_desc& d, bool static_grp) {
    const uint64_t LA = d.LA, LB = d.LB, nA = d.nA, nB = d.nB;
    if (d.direct) {
        const uint64_t ngrp = (nA + 31) / 32;
        return {{"cnt", d.o_cnt, kCntWords, 4},  {"used", d.o_used, d.Lc, 1},     {"lstA", d.o_lstA, 2 * LA + nA, 1},
                {"lstB", d.o_lstB, 2 * LB + nB, 1}, {"neA", d.o_neA, LA, 1},      {"neB", d.o_neB, LB, 1},
                {"icnt", d.o_icnt, 8 * ngrp, 4}, {"iwo", d.o_iwo, ngrp, 1},       {"wle", d.o_wle, nA, 1},
                {"wln", d.o_wln, LA, 1},         {"imask", d.o_imask, 4 * nA, 4}};
    }
    const uint64_t hcap = static_grp ? 0 : 1ull << d.hbits;
    return {{"cnt", d.o_cnt, kCntWords, 4},
            {"hkey", d.o_hkey, 2 * hcap, 2},
            {"hhead", d.o_hhead, hcap, 1},
            {"bmask", d.o_bmask, 2 * d.nblk, 2},
            {"bcnt", d.o_bcnt, 0, 1},
            {"used", d.o_used, d.Lc, 1},
            {"tkey", d.o_tkey, d.S, 1},
            {"lstA", d.o_lstA, 2 * LA + nA, 1},
            {"lstB", d.o_lstB, 2 * LB + nB, 1},
            {"neA", d.o_neA, LA, 1},
            {"neB", d.o_neB, LB, 1},
            {"defer", d.o_defer, LB <= kLaMaxLB ? LA * LB : 0, 1},
            {"info", d.o_info, d.S, 1},
            {"sums", d.o_sums, 8 * d.S, 4},
            {"nxt", d.o_nxt, static_grp ? 0 : d.S, 1},
            {"tb", d.o_tb, d.S, 1},
            {"within", d.o_within, d.S, 1},
            {"etot", d.o_etot, d.S, 1},
            {"cpos", d.o_cpos, d.S, 1},
            {"order", d.o_order, d.capE, 1},
            {"hpos", d.o_hpos, d.capE, 1},
            {"icnt", d.o_icnt, d.iblk ? nA : 0, 1},
            {"imask", d.o_imask, d.iblk ? 4 * nA : 0, 4}};
}

void check_layout(const large_desc& d, bool static_grp, size_t s) {
    const std::vector<span> a = arrays_of(d, static_grp);
    uint64_t end = 0;
    bool ok = true;
    for (const span& x : a) {
        ok &= x.off % x.align == 0;   // 64-bit arrays on even words, 16-byte arrays on multiples of four
        ok &= x.off >= end;           // in order, no overlap
        end = x.off + x.len;
    }
    ok &= d.o_zero % 4 == 0 && d.words % 4 == 0;
    ok &= ((end + 3) & ~3ull) == d.words;   // they end at words
    // the zeroed block covers cnt through used
    ok &= d.o_zero == d.o_cnt && d.o_zero + d.zero_words == d.o_used + d.Lc;
    if (!ok) {
        std::printf("FAILED layout of shape %zu\n", s);
        ++g_failed;
    }
}

void check_rebase(const large_desc& d, size_t s) {
    const uint64_t b = 0x123456789ull;
    large_desc r = d;
    rebase_desc(r, b);
    uint64_t f0[kF], f1[kF];
    fields(d, f0);
    fields(r, f1);
    for (int k = 0; k < kF; ++k) {
        const bool offset = k >= kFirstOffset && k != 20 && k != 47;   // every o_* field and nothing else
        if (f1[k] != f0[k] + (offset ? b : 0)) {
            std::printf("FAILED rebase of shape %zu: %s\n", s, kFieldNames[k]);
            ++g_failed;
        }
    }
}

void check_descs() {
    for (size_t s = 0; s < kNumShapes; ++s) {
        const shape& h = kShapes[s];
        large_desc d;
        std::string why;
        const int rc = build_large_desc(d, 7 + s, h.LA, h.LB, h.nA, h.nB, h.Bm, why, h.sg, h.ad);
        if (s >= kNumAccepted) {
            CHECK(rc == PVAC_ENOSYS && !why.empty());
            continue;
        }
        CHECK(rc == PVAC_OK && (int64_t)kDescExp[s][0] == 0);
        uint64_t f[kF];
        fields(d, f);
        for (int k = 0; k < kF; ++k)
            if (f[k] != kDescExp[s][1 + k]) {
                std::printf("FAILED shape %zu: %s = %llu, expected %llu\n", s, kFieldNames[k], (unsigned long long)f[k],
                            (unsigned long long)kDescExp[s][1 + k]);
                ++g_failed;
            }
        check_layout(d, h.sg, s);
        check_rebase(d, s);
    }
    // what the shapes are there for
    auto built = [](size_t s) {
        large_desc d;
        std::string why;
        const shape& h = kShapes[s];
        build_large_desc(d, 0, h.LA, h.LB, h.nA, h.nB, h.Bm, why, h.sg, h.ad);
        return d;
    };
    CHECK(built(0).iblk == 0 && built(2).iblk == 1 && built(2).direct == 0 && built(3).direct == 1);
    CHECK(built(4).direct == 1 && built(5).direct == 0 && built(5).iblk == 1);
    CHECK(built(6).iblk == 1 && built(7).iblk == 0);
    CHECK(built(8).direct == 1 && built(9).iblk == 0);
    CHECK(built(22).o_info - built(22).o_defer == 9 * 2 && built(9).o_info == built(9).o_defer);   // [LA LB] at LB <= 4
    CHECK(built(10).direct == 1 && built(11).direct == 0 && built(11).iblk == 1);
    CHECK(built(12).direct == 1 && built(13).direct == 0);
    CHECK(built(16).direct == 1 && built(17).direct == 0 && built(17).iblk == 1);
    CHECK(built(18).n == 0 && built(18).capE == 0);
    // the LDS bound of the direct mode, one definition for host and kernel (common.hpp)
    CHECK(dir_lds_bytes(337, 12) == 157648 && dir_lds_bytes(337, 13) == 169712);
    CHECK(dir_lds_bytes(1024, 3) == 135168 && dir_lds_bytes(1024, 4) == 169216);
    CHECK(bucket_count_after_reserve(0) == 2 && bucket_count_after_reserve(6400) == 6427 &&
          bucket_count_after_reserve(3840000) == 4026031);
    CHECK(ceil_log2(0) == 0 && ceil_log2(1) == 0 && ceil_log2(2) == 1 && ceil_log2(3) == 2 && ceil_log2(1024) == 10 &&
          ceil_log2(1025) == 11);
}

// ---------------------------------------------------------------- shared buckets
void check_share() {
    CHECK(slots_share_bucket(97, 98, 7));        // more slots than buckets
    CHECK(slots_share_bucket(6427, 2696, 337));  // chain step 2 (shape 4's bucket count): a collision
    CHECK(!slots_share_bucket(6427, 1348, 337)); // shape 6: none
    CHECK(!slots_share_bucket(6421, 2696, 337));
    CHECK(slots_share_bucket(49157, 2696, 337) && !slots_share_bucket(49157, 674, 337));
    // memoised: the same keys again
    CHECK(slots_share_bucket(6427, 2696, 337) && !slots_share_bucket(6427, 1348, 337));
}

// ---------------------------------------------------------------- cuts
// sets of pairs as indices into kShapes; pair k of a set has id 3 k + 1 and, when its shape has
// static groups, g_head = 1000 k and g_next = 1000 k + S (what the runtime's group tables would give)
const std::vector<int> kSetMixed = {4, 9, 21, 20, 23, 22};   // direct, LB > 4, iblk, dynamic, direct, iblk
const std::vector<int> kSetDirect = {4, 23, 3};

std::vector<large_desc> make_set(const std::vector<int>& idx) {
    std::vector<large_desc> s(idx.size());
    for (size_t k = 0; k < idx.size(); ++k) {
        const shape& h = kShapes[idx[k]];
        std::string why;
        if (build_large_desc(s[k], 3 * k + 1, h.LA, h.LB, h.nA, h.nB, h.Bm, why, h.sg, h.ad)) std::abort();
        if (h.sg) {
            s[k].g_head = 1000 * k;
            s[k].g_next = 1000 * k + s[k].S;
        }
    }
    return s;
}

uint64_t fnv(const void* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t k = 0; k < n; ++k) h = (h ^ ((const uint8_t*)p)[k]) * 0x100000001b3ull;
    return h;
}

// end, words, n_iblk, n_direct, then sizing: nl, n_la, max_S, max_zero, max_tasks, max_capE, max_lay,
// max_tasks_all, max_la_wg, max_nA, any_dyn, all_iblk, any_direct, all_direct, dir_lb, la_per_wg, la_xcd;
// then FNV-1a of the rebased descriptors' bytes and of sel's
constexpr int kC = 23;
const char* const kCutNames[kC] = {"end", "words", "n_iblk", "n_direct", "nl", "n_la", "max_S", "max_zero", "max_tasks",
                                   "max_capE", "max_lay", "max_tasks_all", "max_la_wg", "max_nA", "any_dyn", "all_iblk",
                                   "any_direct", "all_direct", "dir_lb", "la_per_wg", "la_xcd", "desc bytes", "sel bytes"};
const uint64_t kCutExp[][kC] = {
    // mixed, budget 1: the first pair goes alone
    {1, 2100ull, 1ull, 1ull, 1, 1, 0, 33, 0, 0, 17, 8, 1, 0, 0, 1, 1, 1, 1, 8, 0,
     0x6fa4a59c708476e4ull, 0x4d25767f9dce13f5ull},
    // sel: 0
    // mixed, budget = two pairs' words
    {2, 124732ull, 1ull, 1ull, 2, 1, 6740, 1045, 20, 13480, 29, 20, 1, 0, 0, 0, 1, 0, 1, 8, 0,
     0x665075a333a320d4ull, 0x08cd4c29d1e47d34ull},
    // sel: 0 1
    // mixed, one word less
    {1, 2100ull, 1ull, 1ull, 1, 1, 0, 33, 0, 0, 17, 8, 1, 0, 0, 1, 1, 1, 1, 8, 0,
     0x6fa4a59c708476e4ull, 0x4d25767f9dce13f5ull},
    // sel: 0
    // mixed, everything
    {6, 395480ull, 4ull, 2ull, 6, 4, 6740, 25057, 20, 13480, 29, 20, 2, 500, 1, 0, 1, 0, 1, 8, 0,
     0xe8903f31e30bdbccull, 0x2908ae4c1d0f7224ull},
    // sel: 0 2 4 5 1 3
    // mixed, half of everything's words (the out-of-memory split)
    {3, 150432ull, 2ull, 1ull, 3, 2, 6740, 1045, 20, 13480, 29, 20, 1, 96, 0, 0, 1, 0, 1, 8, 0,
     0x23ab9a5b51ff8cdcull, 0xf26292e3dcb93c46ull},
    // sel: 0 2 1
    // mixed from pair 2
    {6, 270748ull, 3ull, 1ull, 4, 3, 6066, 25057, 18, 12132, 29, 18, 2, 500, 1, 0, 1, 0, 1, 8, 0,
     0x49feae0bc9eafbf6ull, 0xb5b17de74c03b3f5ull},
    // sel: 0 2 3 1
    // all direct
    {3, 2804ull, 3ull, 3ull, 3, 3, 0, 33, 0, 0, 17, 8, 1, 0, 0, 1, 1, 1, 1, 8, 0,
     0x8ab60942d367ce32ull, 0x756241e1be8c9396ull},
    // sel: 0 1 2
    // 65,536 minimum pairs: the cap
    {65535, 2883540ull, 65535ull, 65535ull, 65535, 65535, 0, 19, 0, 0, 3, 1, 1, 0, 0, 1, 1, 1, 1, 8, 0,
     0xe5d40eaedf184645ull, 0xb4b45a9ba3bbaccfull},
    // ... and the last one
    {65536, 44ull, 1ull, 1ull, 1, 1, 0, 19, 0, 0, 3, 1, 1, 0, 0, 1, 1, 1, 1, 8, 0,
     0x0543477e35db3f56ull, 0x4d25767f9dce13f5ull},
    // sel: 0
};

// the sizing fields are the only ones cut_sub_batch may set: everything else of mul_large_args zero
bool only_sizing(const mul_large_args& a) {
    mul_large_args z, zero;
    std::memcpy(&z, &a, sizeof z);
    std::memset(&zero, 0, sizeof zero);
    z.nl = z.n_la = 0;
    z.max_S = z.max_zero = z.max_tasks = z.max_capE = z.max_lay = z.max_tasks_all = z.max_la_wg = z.max_nA = 0;
    z.any_dyn = z.all_iblk = z.any_direct = z.all_direct = z.dir_lb = z.la_per_wg = z.la_xcd = 0;
    return std::memcmp(&z, &zero, sizeof z) == 0;
}

bool same(const sub_batch& x, const sub_batch& y) {
    return x.desc.size() == y.desc.size() && x.sel == y.sel && x.words == y.words && x.end == y.end &&
           x.n_iblk == y.n_iblk && x.n_direct == y.n_direct &&
           std::memcmp(x.desc.data(), y.desc.data(), x.desc.size() * sizeof(large_desc)) == 0 &&
           std::memcmp(&x.sizing, &y.sizing, sizeof x.sizing) == 0;
}

// one cut against its row, the properties every cut has, and `out` reused == a fresh sub_batch
void check_cut(const std::vector<large_desc>& set, size_t i, uint64_t budget, int row, sub_batch& out,
               const std::vector<uint32_t>* sel_exp = nullptr) {
    const std::vector<large_desc> before = set;
    cut_sub_batch(set, i, budget, out);
    CHECK(std::memcmp(before.data(), set.data(), set.size() * sizeof(large_desc)) == 0);   // the set is an input
    sub_batch fresh;
    cut_sub_batch(set, i, budget, fresh);
    CHECK(same(out, fresh));
    const mul_large_args& a = out.sizing;
    const uint64_t got[kC] = {out.end, out.words, out.n_iblk, out.n_direct, a.nl, a.n_la, a.max_S, a.max_zero, a.max_tasks,
                              a.max_capE, a.max_lay, a.max_tasks_all, a.max_la_wg, a.max_nA, a.any_dyn, a.all_iblk,
                              a.any_direct, a.all_direct, a.dir_lb, a.la_per_wg, a.la_xcd,
                              fnv(out.desc.data(), out.desc.size() * sizeof(large_desc)),
                              fnv(out.sel.data(), out.sel.size() * sizeof(uint32_t))};
    for (int k = 0; k < kC; ++k)
        if (got[k] != kCutExp[row][k]) {
            std::printf("FAILED cut %d: %s = %llu, expected %llu\n", row, kCutNames[k], (unsigned long long)got[k],
                        (unsigned long long)kCutExp[row][k]);
            ++g_failed;
        }
    CHECK(only_sizing(a));
    if (sel_exp) CHECK(out.sel == *sel_exp);
    // the rules, whatever the numbers
    const size_t n = out.end - i;
    CHECK(out.end > i && n <= 65535 && out.desc.size() == n && out.sel.size() == n && a.nl == n);
    CHECK(a.dir_lb >= 1 && a.la_xcd == 0 && a.la_per_wg == kLaPerWG);
    uint64_t w = 0, mS = 0, mE = 0, mA = 0, mL = 0;
    bool ok = true;
    for (size_t k = 0; k < n; ++k) {
        large_desc r = set[i + k];   // the descriptors: the set's, laid end to end from word 0
        rebase_desc(r, w);
        ok &= std::memcmp(&r, &out.desc[k], sizeof r) == 0;
        w += r.words;
        if (!r.direct) {   // direct pairs do not count toward max_S, max_capE, max_nA
            mS = std::max(mS, r.S);
            mE = std::max(mE, r.capE);
            mA = std::max<uint64_t>(mA, r.iblk ? r.nA : 0);
        }
        mL = std::max<uint64_t>(mL, std::max<uint64_t>(r.Lc, (uint64_t)r.LA + r.LB));
    }
    CHECK(ok && w == out.words);
    CHECK(a.max_S == mS && a.max_capE == mE && a.max_nA == mA && a.max_lay == mL);
    CHECK(n == 1 || out.words <= budget);   // only the first pair may exceed the budget
    CHECK(out.end == set.size() || n == 65535 || out.words + set[out.end].words > budget);   // and it is greedy
    // sel: a permutation, the LB <= kLaMaxLB class first, each class ascending
    ok = a.n_la <= n;
    for (size_t k = 0; k < n && ok; ++k) {
        ok &= out.sel[k] < n && (out.desc[out.sel[k]].LB <= kLaMaxLB) == (k < a.n_la);
        ok &= k == 0 || k == a.n_la || out.sel[k] > out.sel[k - 1];
    }
    CHECK(ok);
}

void check_cuts() {
    const std::vector<large_desc> mixed = make_set(kSetMixed), direct = make_set(kSetDirect);
    const std::vector<large_desc> many = make_set(std::vector<int>(65536, 3));
    uint64_t all = 0;
    for (const large_desc& d : mixed) all += d.words;
    sub_batch sb;   // one object through every cut: its storage is reused
    const std::vector<uint32_t> one = {0};
    check_cut(mixed, 0, 1, 0, sb, &one);                                        // below the first pair's words
    CHECK(sb.end == 1);
    const std::vector<uint32_t> two = {0, 1};
    check_cut(mixed, 0, mixed[0].words + mixed[1].words, 1, sb, &two);          // exactly two pairs' words
    CHECK(sb.end == 2);
    check_cut(mixed, 0, mixed[0].words + mixed[1].words - 1, 2, sb, &one);      // one word less
    CHECK(sb.end == 1);
    const std::vector<uint32_t> sel_all = {0, 2, 4, 5, 1, 3};
    check_cut(mixed, 0, 1ull << 60, 3, sb, &sel_all);
    CHECK(sb.end == 6 && sb.words == all && sb.sizing.n_la == 4 && sb.n_direct == 2 && sb.n_iblk == 4);
    CHECK(sb.sizing.any_dyn == 1 && sb.sizing.all_iblk == 0 && sb.sizing.any_direct == 1 && sb.sizing.all_direct == 0);
    // the out-of-memory split: the same start with half the words
    const sub_batch whole = sb;
    const std::vector<uint32_t> sel_half = {0, 2, 1};
    check_cut(mixed, 0, std::max<uint64_t>(whole.words / 2, 1), 4, sb, &sel_half);
    CHECK(sb.end < whole.end && sb.end == 3);
    const std::vector<uint32_t> sel_tail = {0, 2, 3, 1};
    check_cut(mixed, 2, 1ull << 60, 5, sb, &sel_tail);
    const std::vector<uint32_t> sel_dir = {0, 1, 2};
    check_cut(direct, 0, 1ull << 60, 6, sb, &sel_dir);
    CHECK(sb.sizing.all_direct == 1 && sb.sizing.max_S == 0 && sb.sizing.max_capE == 0 && sb.sizing.max_nA == 0);
    check_cut(many, 0, 1ull << 60, 7, sb);                                      // the 65,535-pair cap
    CHECK(sb.end == 65535);
    check_cut(many, 65535, 1ull << 60, 8, sb, &one);
    CHECK(sb.end == 65536);
}

}  // namespace

int main() {
    check_descs();
    check_share();
    check_cuts();
    if (g_failed) {
        std::printf("large_plan_check: %d FAILED\n", g_failed);
        return 1;
    }
    std::printf("large_plan_check: ok\n");
    return 0;
}
