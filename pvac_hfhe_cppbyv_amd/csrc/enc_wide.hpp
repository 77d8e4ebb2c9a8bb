// enc_wide.hpp — the table logic of the wide encryption route (k_enc_wide.hip) and its host-side
// sizing (rt_keys.cpp), in one place so that the kernels, the runtime and the CPU check
// (tests/cpp/enc_wide_check.cpp) state it once. No HIP types: a plain C++ compiler reads this file.
//
// A half (one enc_fp_depth) has npre = 8 + 2 Z2 + 3 Z3 pre-merge edges in creation order, each with a
// key (idx, ch); compact_edges (reference ops/encrypt.hpp:39-71) merges the edges of equal keys and
// emits the merged edges sorted by (idx, P before M). The narrow route (enc_dev.hpp::plan_half) finds
// the groups by comparing every edge with every other. Here a half owns a table of 2 B words, one
// per key sk = 2 idx + ch, in global scratch, and three linear steps:
//   1. wide_note, by the lane that replays the draws, per edge in creation order: the edge's
//      occurrence number among the edges of its key (0 = the key's first occurrence), and the key's
//      count in the table. The number of first occurrences is nout, which the shuffle needs before
//      the next half of a VALUE item can draw.
//   2. a scan over the 2 B keys (by a workgroup): a present key's rank = the present keys below it,
//      its segment start = the edges of the keys below it. wide_place_key records both.
//   3. wide_place_edge, per edge, in any order: its place in the stable counting sort is its key's
//      start plus its occurrence number, so a group's segment lists its contributors in creation order.
// wide_group_host runs the three steps on the CPU with the same functions.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define PVW_HD __host__ __device__
#else
#define PVW_HD
#endif

namespace pvhip {

// pre-merge edges per half the narrow kernels hold (kEncPreMax) = the default plan limit
constexpr uint32_t kEncPlanLimitDefault = 256;
constexpr uint32_t kEncPlanLimitMax = 1u << 24;
constexpr uint64_t kEncBudgetDefault = 1ull << 22;   // pre-merge edges of a sub-batch
constexpr uint32_t kEncWideFinChunk = 16;            // output edges a finish workgroup is dealt

PVW_HD inline uint32_t wide_sk(uint32_t key) { return (key & 0xFFFFu) * 2u + (key >> 16); }   // key = idx | ch << 16

// step 1: the occurrence number of an edge with this key; tab (2 B words) starts zeroed
PVW_HD inline uint32_t wide_note(uint32_t* tab, uint32_t key) {
    const uint32_t k = wide_sk(key), c = tab[k];
    tab[k] = c + 1;
    return c;
}
// step 2: key k is present, `rank` present keys and `start` edges lie below it
PVW_HD inline void wide_place_key(uint32_t* tab, uint32_t* gstart, uint32_t k, uint32_t rank, uint32_t start) {
    gstart[rank] = start;
    tab[k] = start;
}
// step 3: edge e into the sorted order
PVW_HD inline void wide_place_edge(const uint32_t* tab, const uint32_t* key, const uint32_t* occ, uint32_t* ord, uint32_t e) {
    ord[tab[wide_sk(key[e])] + occ[e]] = e;
}
// group g's contributors are ord[b .. e)
PVW_HD inline void wide_segment(const uint32_t* gstart, uint32_t nout, uint32_t npre, uint32_t g, uint32_t& b, uint32_t& e) {
    b = gstart[g];
    e = g + 1 < nout ? gstart[g + 1] : npre;
}

// the three steps in turn; tab holds 2 B zeroed words, occ / gstart / ord npre words. Returns nout.
inline uint32_t wide_group_host(const uint32_t* key, uint32_t npre, uint32_t B, uint32_t* tab, uint32_t* occ, uint32_t* gstart,
                                uint32_t* ord) {
    uint32_t nout = 0;
    for (uint32_t e = 0; e < npre; ++e) {
        occ[e] = wide_note(tab, key[e]);
        nout += occ[e] == 0;
    }
    uint32_t rank = 0, start = 0;
    for (uint32_t k = 0; k < 2 * B; ++k) {
        const uint32_t cnt = tab[k];
        if (!cnt) continue;
        wide_place_key(tab, gstart, k, rank, start);
        ++rank;
        start += cnt;
    }
    for (uint32_t e = 0; e < npre; ++e) wide_place_edge(tab, key, occ, ord, e);
    return nout;
}

// ---- plans and draws
PVW_HD inline uint64_t enc_npre(uint32_t z2, uint32_t z3) { return 8 + 2ull * z2 + 3ull * z3; }

// Draws of one half without rejections: nonce 2, signal 2*8 + 2*7, salts npre, noise picks / signs /
// coefficients 5 Z2 + 10 Z3, shuffle npre (it takes nout - 1 <= npre - 1).
inline uint64_t enc_half_draws(uint32_t z2, uint32_t z3) {
    const uint64_t npre = enc_npre(z2, z3);
    return 2 + 16 + 14 + npre + 5ull * z2 + 10ull * z3 + npre;
}
// The slack of a half's draws_hint. A rejection costs one draw: a signal pick repeats an earlier one
// with probability q/B (q = 0..7, 28/B in all), a pair's second index its first with 1/B, a triple's
// second and third with 1/B and 2/B, and every retry repeats with the same probability. The rejected
// draws of a half are a sum R of geometric counts with failure probabilities q_i <= 7/B and
// mu = sum q_i = (28 + Z2 + 3 Z3) / B. R >= s needs s failures spread over the trials, so by the
// union bound P(R >= s) <= h_s(q), the complete homogeneous polynomial, which is at most the
// coefficient of x^s in exp(mu x / (1 - 7x/B)): about mu^s / s! <= (e mu / s)^s. Up to 256 edges the
// slack is the constant 32 and stays so; its worst case is the hint-124 half with the default Params
// (mu = 207 / 337 = 0.61), where running out needs 33 rejections: (e mu / 33)^33 < 2^-142. Above 256
// edges the slack is s = max(146, ceil(6 mu)): s >= 6 mu > 2 e mu makes (e mu / s)^s <= 2^-s <= 2^-146,
// no higher than that, at any plan. (The shuffle's unused draws add to the slack and are not counted.)
inline uint64_t enc_half_slack(uint32_t z2, uint32_t z3, uint32_t B) {
    if (enc_npre(z2, z3) <= kEncPlanLimitDefault) return 32;
    const uint64_t b = B ? B : 1;
    return std::max<uint64_t>(146, (6 * (28 + (uint64_t)z2 + 3ull * z3) + b - 1) / b);
}
// draws_hint of an item: a bare half, or the mask's two words and two halves
inline uint64_t enc_draws_hint(uint32_t z2, uint32_t z3, uint32_t B, uint32_t halves) {
    const uint64_t half = enc_half_draws(z2, z3), slack = enc_half_slack(z2, z3, B);
    return halves == 2 ? 2 + 2 * half + 2 * slack : half + slack;
}

// ---- sub-batches: consecutive items, cut where the pre-merge total would pass the budget; an item
// above the budget runs alone. cuts = the first item of every sub-batch, then n.
inline void enc_cuts(const uint64_t* item_pe, size_t n, uint64_t budget, std::vector<size_t>& cuts) {
    cuts.clear();
    uint64_t sum = 0;
    for (size_t i = 0; i < n; ++i) {
        if (i == 0 || sum + item_pe[i] > budget) {
            cuts.push_back(i);
            sum = 0;
        }
        sum += item_pe[i];
    }
    cuts.push_back(n);
}

// ---- scratch of one sub-batch on the mixed path (rt_keys.cpp run_enc_sub), byte offsets into the arena
struct enc_sub_shape {
    uint64_t n = 0, n_narrow = 0, n_wide = 0;   // items
    uint64_t halves = 0, pe = 0, cores = 0;     // of all its items
    uint64_t work_narrow = 0, work_wide = 0;    // (half, group) entries
    uint64_t fin = 0;                           // finish chunks of the wide halves
    uint32_t B = 0, sigma_words = 0;            // sigma_words = 0: no sigma
};
struct enc_sub_layout {
    // uploaded in one copy
    uint64_t recs_narrow, recs_wide, nid, wid, perm, work_narrow, work_wide, fin, half_item, up_bytes;
    // device only
    uint64_t hdr, req, core, pre_idx, tmp_idx, tmp_status, lay, e, key, grp, occ, tab, dlast, sig, total;
};
inline uint64_t enc_al(uint64_t b) { return (b + 255) & ~255ull; }
// rec_bytes / hdr_bytes / req_bytes / layer_bytes: sizeof enc_item_rec, enc_half_hdr, prf_request, pvac_layer
inline enc_sub_layout enc_sub_layout_of(const enc_sub_shape& s, uint64_t rec_bytes, uint64_t hdr_bytes, uint64_t req_bytes,
                                        uint64_t layer_bytes) {
    enc_sub_layout L{};
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { const uint64_t at = o; o += enc_al(bytes); return at; };
    L.recs_narrow = take(s.n_narrow * rec_bytes);
    L.recs_wide = take(s.n_wide * rec_bytes);
    L.nid = take(s.n_narrow * 4);
    L.wid = take(s.n_wide * 4);
    L.perm = take(s.n_narrow * 4);
    L.work_narrow = take(s.work_narrow * 8);
    L.work_wide = take(s.work_wide * 8);
    L.fin = take(s.fin * 8);
    L.half_item = take(s.halves * 4);
    L.up_bytes = o;
    L.hdr = take(s.halves * hdr_bytes);
    L.req = take(s.cores * req_bytes);
    L.core = take(s.cores * 16);
    L.pre_idx = take(s.n * 32);
    L.tmp_idx = take(s.n_narrow * 32);
    L.tmp_status = take(s.n_narrow * 4);
    L.lay = take(s.halves * layer_bytes);
    L.e = take(s.pe * 48);                         // meta, w_lo, w_hi, salt, rlo, rhi
    L.key = take(s.pe * 4);
    L.grp = take(s.n_narrow ? s.pe * 2 : 0);       // narrow: grp, slot (bytes)
    L.occ = take(s.n_wide ? s.pe * 16 : 0);        // wide: occ, ord, gstart, slot (words)
    L.tab = take(s.n_wide * 2 * 2 * (uint64_t)s.B * 4);   // two tables of 2 B words per wide item
    L.dlast = take(s.n_wide ? s.halves * 16 : 0);
    L.sig = take(s.pe * s.sigma_words * 8);
    L.total = o;
    return L;
}

}  // namespace pvhip
