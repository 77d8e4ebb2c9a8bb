// large_plan.hpp — host-side planning of the general ct_mul path (k_mul_large.hip): a pair's scratch
// layout, and the cut of a planned pair set into sub-batches that fit a scratch budget. Pure
// arithmetic over the types of common.hpp: no HIP runtime calls, checked without a GPU
// (tests/cpp/large_plan_check.cpp).
#pragma once
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "common.hpp"

namespace pvhip {

// libstdc++ bucket count chosen by std::unordered_map::reserve(n) on an empty map: the
// container rehashes to _M_next_bkt(max(1, ceil(n / max_load_factor))) with max load 1.0.
// Asking the policy object directly gives the identical value without allocating.
inline uint64_t bucket_count_after_reserve(uint64_t n) {
    std::__detail::_Prime_rehash_policy pol(1.0f);
    const uint64_t want = std::max<uint64_t>(1, (uint64_t)pol._M_bkt_for_elements(n));
    return pol._M_next_bkt(want);
}

inline uint32_t ceil_log2(uint64_t x) {
    uint32_t b = 0;
    while ((1ull << b) < x) ++b;
    return b;
}

// A pair beyond the LDS layer tables of k_large_lists / k_large_layers (accepted only under a raised
// layer limit, pvac_hip_ctx_set_layer_limit)
inline bool is_deep(const large_desc& d) { return d.Lc > kLargeLayersMax; }

// Scratch layout of one general-path pair (k_mul_large.hip), offsets relative to 0; the
// executor rebases them into the arena. 64-bit arrays on even words, 16-byte arrays on
// multiples of four.
inline int build_large_desc(large_desc& d, uint64_t pair, uint64_t LA, uint64_t LB, uint64_t nA, uint64_t nB, uint32_t Bm,
                            std::string& why, bool static_grp = false, bool allow_direct = false,
                            uint32_t layers_max = kLargeLayersMax) {
    d = large_desc{};
    d.pair = pair;
    d.n = nA * nB;
    d.S = LA * LB * Bm;
    d.Lc = LA + LB + LA * LB;
    if (LA > 0xFFFFFFFFull || LB > 0xFFFFFFFFull || nA > 0xFFFFFFFFull || nB > 0xFFFFFFFFull ||
        (nA && d.n / nA != nB) || d.n >= (1ull << 32)) {
        why = "ct_mul: |A.E||B.E| >= 2^32 products in one pair";
        return PVAC_ENOSYS;
    }
    if (d.Lc > layers_max) {
        why = "ct_mul: more than " + std::to_string(layers_max) + " layers before compaction in one pair";
        return PVAC_ENOSYS;
    }
    // a deep pair (k_large_deep.hip: its layer tables in global scratch) takes the dynamic route only:
    // the iblk order, the direct mode and the static groups pack a layer into 15 or 16 bits
    if (is_deep(d)) static_grp = allow_direct = false;
    if (d.S >= (1ull << 31)) {
        why = "ct_mul: key space |A.L||B.L|B >= 2^31";
        return PVAC_ENOSYS;
    }
    d.LA = (uint32_t)LA; d.LB = (uint32_t)LB; d.nA = (uint32_t)nA; d.nB = (uint32_t)nB;
    d.nblk = (d.n + 15) / 16;
    const uint64_t keys = std::min(d.n, d.S);
    d.capE = 2 * keys;
    d.nbm = make_fastmod64(bucket_count_after_reserve(d.n));
    d.hbits = std::max<uint32_t>(1, ceil_log2(2 * std::max<uint64_t>(keys, 1)));
    d.g_head = d.g_next = kNoGrp;
    // per-A-edge emit order (k_large_products.hip): static groups and the A-layer-major products kernel
    d.iblk = static_grp && LB <= kLaMaxLB && nA >= 1 && nB >= 1 && nB <= kIblkMaxNB ? 1u : 0u;
    // (direct A ids and writer lists pack an A edge with its dense cell: A edges < 2^21, 2 B <= 2^11)
    // (and k_large_products_direct's LDS: the digit table, LB staged B layers and their sums)
    d.direct = d.iblk && allow_direct && nA < (1ull << 21) && Bm <= 1024u &&
                       dir_lds_bytes(Bm, (uint32_t)LB) <= 160u * 1024u
                   ? 1u
                   : 0u;
    d.nb_m = nB ? (1ull << 32) / nB : 0;
    uint64_t o = 0;
    auto even = [&]() { o = (o + 1) & ~1ull; };
    auto quad = [&]() { o = (o + 3) & ~3ull; };
    if (d.direct) {
        // no per-key scratch: cnt | used, the edge lists, per-A-edge counts and masks
        quad();
        d.o_zero = d.o_cnt = o;
        o += kCntWords;
        d.o_hkey = d.o_hhead = d.o_bmask = o;
        d.o_bcnt = d.o_used = o;
        o += d.Lc;
        d.zero_words = o - d.o_zero;
        d.o_tkey = o;
        d.o_lstA = o; o += 2 * LA + nA;
        d.o_lstB = o; o += 2 * LB + nB;
        d.o_neA = o; o += LA;
        d.o_neB = o; o += LB;
        d.o_defer = d.o_info = d.o_sums = d.o_nxt = d.o_tb = d.o_within = d.o_etot = d.o_cpos = d.o_order = d.o_hpos = o;
        const uint64_t ngrp = (nA + 31) / 32;
        quad();
        d.o_icnt = o; o += 8 * ngrp;   // count bytes
        d.o_iwo = o; o += ngrp;
        d.o_wle = o; o += nA;
        d.o_wln = o; o += LA;
        quad();
        d.o_imask = o; o += 4 * nA;
        quad();
        d.words = o;
        return PVAC_OK;
    }
    const uint64_t hcap = static_grp ? 0 : 1ull << d.hbits;   // static groups: no bucket table / chains
    quad();
    d.o_zero = o;
    d.o_cnt = o; o += kCntWords;
    d.o_hkey = o; o += 2 * hcap;
    d.o_hhead = o; o += hcap;
    even();
    d.o_bmask = o; o += 2 * d.nblk;
    d.o_bcnt = o;
    d.o_used = o; o += d.Lc;
    d.zero_words = o - d.o_zero;
    d.o_tkey = o; o += d.S;
    d.o_lstA = o; o += 2 * LA + nA;
    d.o_lstB = o; o += 2 * LB + nB;
    d.o_neA = o; o += LA;
    d.o_neB = o; o += LB;
    d.o_defer = o; o += LA * LB <= kLaMaxLB * LA ? LA * LB : 0;   // A-layer-major pairs only
    d.o_info = o; o += d.S;
    quad();
    d.o_sums = o; o += 8 * d.S;
    d.o_nxt = o; o += static_grp ? 0 : d.S;
    d.o_tb = o; o += d.S;
    d.o_within = o; o += d.S;
    d.o_etot = o; o += d.S;
    d.o_cpos = o; o += d.S;
    d.o_order = o; o += d.capE;
    d.o_hpos = o; o += d.capE;
    d.o_icnt = o; o += d.iblk ? nA : 0;
    quad();
    d.o_imask = o; o += d.iblk ? 4 * nA : 0;
    quad();
    d.o_wle = d.o_wln = d.o_iwo = o;
    d.words = o;
    return PVAC_OK;
}

inline void rebase_desc(large_desc& d, uint64_t base) {
    uint64_t* f[] = {&d.o_zero, &d.o_cnt, &d.o_hkey, &d.o_hhead, &d.o_bmask, &d.o_bcnt, &d.o_used, &d.o_tkey,
                     &d.o_lstA, &d.o_lstB, &d.o_neA, &d.o_neB, &d.o_defer, &d.o_info, &d.o_sums, &d.o_nxt, &d.o_tb,
                     &d.o_within, &d.o_etot, &d.o_cpos, &d.o_order, &d.o_hpos, &d.o_icnt, &d.o_imask,
                     &d.o_wle, &d.o_wln, &d.o_iwo};
    // every o_* field is in the list (zero_words and words are sizes and stay); a new one belongs here
    static_assert(sizeof(large_desc) == 352, "large_desc changed: visit rebase_desc's field list");
    for (uint64_t* p : f) *p += base;
}

// Whether two key slots of [0, S) share a libstdc++ bucket among nb buckets (std::hash<u64> times the
// reference's 0x9E3779B97F4A7C15, arithmetic.hpp:72-77). A pair whose slots can share a bucket is not
// taken in the direct mode (its emit order then needs bucket leaders across A layers): chain step 2
// (|A.L| = 8, bucket counts near 49 K) has hundreds of such buckets, deeper steps none (the structured
// keys (lp << 32) | r spread perfectly there). Memoised per (nb, S, B): chunks of one step repeat them,
// and the slot -> key map depends on B (two contexts with different B can meet the same (nb, S)).
inline bool slots_share_bucket(uint64_t nb, uint64_t S, uint32_t Bm) {
    static std::mutex mu;
    static std::map<std::tuple<uint64_t, uint64_t, uint32_t>, bool> memo;
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = memo.find({nb, S, Bm});
        if (it != memo.end()) return it->second;
    }
    bool shared = false;
    if (S > nb) {
        shared = true;
    } else {
        std::vector<uint64_t> seen((nb + 63) / 64, 0);
        for (uint64_t s = 0; s < S && !shared; ++s) {
            const uint64_t key = ((s / Bm) << 32) | (s % Bm);
            const uint64_t b = (key * kGolden) % nb;
            const uint64_t m = 1ull << (b & 63);
            shared = (seen[b >> 6] & m) != 0;
            seen[b >> 6] |= m;
        }
    }
    std::lock_guard<std::mutex> g(mu);
    memo[{nb, S, Bm}] = shared;
    return shared;
}

// One launch_ct_mul_large: the pairs set[i, end) with their scratch laid end to end from arena word 0.
struct sub_batch {
    std::vector<large_desc> desc;   // set[i, end), rebased (storage reused from call to call)
    std::vector<uint32_t> sel;      // descriptor order of the products kernels: the A-layer-major class
                                    // (|B.L| <= kLaMaxLB) first, each class in pair order
    uint64_t words = 0;             // arena words the sub-batch needs
    size_t end = 0;
    uint32_t n_iblk = 0, n_direct = 0;   // path counters
    // launch sizing only: nl, n_la, max_*, any_dyn, all_iblk, any_direct, all_direct, dir_lb, la_per_wg,
    // la_xcd; the caller fills in the pointers and the context's parameters
    mul_large_args sizing{};
};

// Cuts the sub-batch that starts at set[i]: pairs are taken while their scratch fits `budget` words,
// the first one always (a pair larger than the budget runs alone), at most 65,535 (the grid-y limit).
// Deep pairs get sub-batches of their own (another launch sequence): a sub-batch ends where deepness changes.
// `set` is left as it is; the out-of-memory split is a second call with a smaller budget.
inline void cut_sub_batch(const std::vector<large_desc>& set, size_t i, uint64_t budget, sub_batch& out) {
    out.n_iblk = out.n_direct = 0;
    mul_large_args& a = out.sizing;
    a = mul_large_args{};
    a.all_iblk = a.all_direct = 1u;
    uint64_t words = 0;
    size_t j = i;
    const bool deep = i < set.size() && is_deep(set[i]);
    while (j < set.size() && (j == i || words + set[j].words <= budget) && j - i < 65535 && is_deep(set[j]) == deep)
        words += set[j++].words;
    out.desc.assign(set.begin() + i, set.begin() + j);
    uint64_t base = 0;
    for (large_desc& d : out.desc) {
        rebase_desc(d, base);
        base += d.words;   // (rebase_desc leaves it the pair's own size)
        // direct pairs have no per-key scratch: the slot- and edge-sized grids are the others'
        if (!d.direct) {
            a.max_S = std::max(a.max_S, d.S);
            a.max_capE = std::max(a.max_capE, d.capE);
            a.max_nA = std::max<uint64_t>(a.max_nA, d.iblk ? d.nA : 0);
        }
        a.max_zero = std::max(a.max_zero, d.zero_words);
        a.any_dyn |= d.g_head == kNoGrp ? 1u : 0u;
        a.all_iblk &= d.iblk != 0 ? 1u : 0u;
        a.any_direct |= d.direct != 0 ? 1u : 0u;
        a.all_direct &= d.direct != 0 ? 1u : 0u;
        out.n_iblk += d.iblk;
        out.n_direct += d.direct;
        if (d.direct) a.dir_lb = std::max<uint32_t>(a.dir_lb, d.LB);
        a.max_lay = std::max(a.max_lay, std::max<uint64_t>(d.Lc, (uint64_t)d.LA + d.LB));
        if (deep) a.max_nA = std::max<uint64_t>(a.max_nA, std::max(d.nA, d.nB));   // (never iblk: see mul_large_args::deep)
    }
    a.deep = deep ? 1u : 0u;
    // k_large_products_la's deferred-task list packs an A layer index into 16 bits: a (deep) pair of
    // 2^16 A layers or more takes one workgroup per task
    auto la_class = [](const large_desc& d) { return d.LB <= kLaMaxLB && d.LA < (1u << 16); };
    // products: pairs with few B layers (chain steps) take the A-layer-major kernel
    const size_t n = j - i;
    out.sel.resize(n);
    for (size_t k = 0; k < n; ++k)
        if (la_class(out.desc[k])) out.sel[a.n_la++] = (uint32_t)k;
    for (size_t k = 0, q = a.n_la; k < n; ++k) {
        const large_desc& d = out.desc[k];
        const uint64_t tasks = (uint64_t)d.LA * d.LB;
        a.max_tasks_all = std::max(a.max_tasks_all, tasks);
        if (la_class(d)) {
            a.max_la_wg = std::max<uint64_t>(a.max_la_wg, (d.LA + kLaPerWG - 1) / kLaPerWG);
        } else {
            a.max_tasks = std::max(a.max_tasks, tasks);
            out.sel[q++] = (uint32_t)k;
        }
    }
    a.nl = (uint32_t)n;
    a.dir_lb = std::max<uint32_t>(a.dir_lb, 1u);
    a.la_per_wg = kLaPerWG;
    a.la_xcd = 0;
    out.words = words;
    out.end = j;
}

}  // namespace pvhip
