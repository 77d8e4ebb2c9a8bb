// test_deep_ops.cpp — ct_sum / ct_lincomb_batch, compact_edges and ct_recrypt of ciphers of more than
// 30,000 layers through the C++ adapter (include/pvac_hip.hpp), on types that mirror the reference's field
// layout (core/types.hpp:72-139), on an engine whose layer limit was raised with set_layer_limit. The
// ciphers are built here (many layer records, a few edges), in shapes whose results can be stated
// directly: a heap of PROD layers keeps every layer, distinct (layer, idx, ch) cells merge nothing.
// Runs on the GPU box: test_deep_ops. Exit 0 = every check passed.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "pvac_hip.hpp"

namespace mirror {   // same member names/types as pvac:: (core/types.hpp, core/field.hpp, core/bitvec.hpp)
struct Fp { uint64_t lo, hi; };
struct BitVec { size_t nbits = 0; std::vector<uint64_t> w; };
struct Nonce128 { uint64_t lo, hi; };
struct RSeed { uint64_t ztag; Nonce128 nonce; };
enum class RRule : uint8_t { BASE = 0, PROD = 1 };
struct Layer { RRule rule; RSeed seed; uint32_t pa; uint32_t pb; };
struct Edge { uint32_t layer_id; uint16_t idx; uint8_t ch; Fp w; BitVec s; };
struct Cipher { std::vector<Layer> L; std::vector<Edge> E; };
struct Params {
    int B = 7, m_bits = 8192, n_bits = 16384, h_col_wt = 192, x_col_wt = 128, err_wt = 128;
    double noise_entropy_bits = 120.0, tuple2_fraction = 0.55, depth_slope_bits = 16.0;
    size_t edge_budget = 1200000;
    int lpn_n = 4096, lpn_t = 16384, lpn_tau_num = 1, lpn_tau_den = 8;
};
struct Ubk { std::vector<int> perm; std::vector<int> inv; };
struct PubKey {
    Params prm; uint64_t canon_tag = 0; std::vector<BitVec> H; Ubk ubk;
    std::array<uint8_t, 32> H_digest{}; std::vector<Fp> powg_B;
};
struct EvalKey { std::vector<Cipher> zero_pool; Cipher enc_one; };
}  // namespace mirror

using mirror::Cipher;
using mirror::Edge;
using mirror::Layer;
using mirror::RRule;

static int g_checks = 0;
#define MUST(cond, ...)                                                        \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);          \
            std::fprintf(stderr, __VA_ARGS__);                                 \
            std::fprintf(stderr, "\n");                                        \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

static uint64_t g_state = 0xD0D0;
static uint64_t rnd64() {   // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

static Edge edge(uint32_t layer, uint16_t idx, uint8_t ch, bool sigma) {
    Edge e{layer, idx, ch, {rnd64(), rnd64() >> 2}, {}};
    if (sigma) {
        e.s.nbits = 8192;
        e.s.w.assign(128, 0);   // all-zero rows: the density is 0, so ct_recrypt runs its eight iterations
    }
    return e;
}

// nl layers as a heap (layer l = PROD of 2l + 1 and 2l + 2 while they exist), an edge on layer 0 and on
// `extra` others, every (layer, idx, ch) cell used once: compact_layers keeps every layer
static Cipher heap(uint32_t nl, uint32_t extra, bool sigma) {
    Cipher c;
    c.L.resize(nl);
    for (uint32_t l = 0; l < nl; ++l) {
        if (2 * l + 1 < nl) c.L[l] = Layer{RRule::PROD, {0, {0, 0}}, 2 * l + 1, std::min(2 * l + 2, nl - 1)};
        else c.L[l] = Layer{RRule::BASE, {rnd64() >> 1, {rnd64(), rnd64()}}, 0, 0};
    }
    c.E.push_back(edge(0, 3, 1, sigma));
    for (uint32_t k = 0; k < extra; ++k) c.E.push_back(edge((uint32_t)(rnd64() % nl), (uint16_t)(k % 7), (uint8_t)(k & 1), sigma));
    return c;
}

static bool same_layer(const Layer& a, const Layer& b, uint32_t shift) {
    if (a.rule != b.rule) return false;
    if (a.rule == RRule::PROD) return a.pa == b.pa + shift && a.pb == b.pb + shift;
    return a.seed.ztag == b.seed.ztag && a.seed.nonce.lo == b.seed.nonce.lo && a.seed.nonce.hi == b.seed.nonce.hi;
}

static bool same_edge(const Edge& a, const Edge& b, uint32_t shift) {
    return a.layer_id == b.layer_id + shift && a.idx == b.idx && a.ch == b.ch && a.w.lo == b.w.lo && a.w.hi == b.w.hi;
}

int main() {
    mirror::PubKey pk;
    pk.canon_tag = 0xD0D1;
    pk.ubk.inv.resize(8192);
    for (int i = 0; i < 8192; ++i) pk.ubk.inv[i] = 8191 - i;
    pvac_hip::Engine& eng = pvac_hip::engine_for(pk);
    eng.set_layer_limit(1u << 17);
    MUST(eng.layer_limit() == (1u << 17), "set_layer_limit");
    MUST(eng.deep_route_counts() == (std::array<uint64_t, 4>{0, 0, 0, 0}), "a new engine has counted nothing");

    const uint32_t nl = 30001;
    const Cipher deep = heap(nl, 20, false), small = heap(5, 3, false);

    // ---- ct_sum: the deep term and a shallow one, each compacted on its own, concatenated
    {
        const Cipher out = pvac_hip::ct_sum(pk, std::vector<Cipher>{deep, small}, false);
        MUST(out.L.size() == nl + 5 && out.E.size() == deep.E.size() + small.E.size(), "ct_sum: %zu layers, %zu edges",
             out.L.size(), out.E.size());
        for (uint32_t l = 0; l < nl; ++l) MUST(same_layer(out.L[l], deep.L[l], 0), "ct_sum: layer %u", l);
        for (uint32_t l = 0; l < 5; ++l) MUST(same_layer(out.L[nl + l], small.L[l], nl), "ct_sum: layer %u of the second term", l);
        for (size_t e = 0; e < deep.E.size(); ++e) MUST(same_edge(out.E[e], deep.E[e], 0), "ct_sum: edge %zu", e);
        for (size_t e = 0; e < small.E.size(); ++e)
            MUST(same_edge(out.E[deep.E.size() + e], small.E[e], nl), "ct_sum: edge %zu of the second term", e);
        MUST(eng.deep_route_counts()[0] == 1, "one term on the deep-term route");
    }
    // ---- ct_lincomb_batch: a flat deep cipher keeps only its edges' layers; scaled by 1 (fp_mul of a canonical word)
    {
        Cipher flat;
        flat.L.resize(nl + 9);
        for (auto& L : flat.L) L = Layer{RRule::BASE, {rnd64() >> 1, {rnd64(), rnd64()}}, 0, 0};
        const uint32_t at[3] = {7, 15000, nl + 8};
        for (int k = 0; k < 6; ++k) flat.E.push_back(edge(at[k % 3], (uint16_t)k, 0, false));
        for (auto& e : flat.E) e.w.hi &= (1ull << 62) - 1;
        const auto out = pvac_hip::ct_lincomb_batch(pk, std::vector<Cipher>{small, flat}, {0, 2, 3}, {0, 1, 1},
                                                    std::vector<mirror::Fp>{{1, 0}, {1, 0}, {1, 0}}, {0, 1, 0}, false);
        MUST(out.size() == 2 && out[0].L.size() == 5 + 3 && out[1].L.size() == 3, "ct_lincomb_batch: layer counts");
        for (int k = 0; k < 6; ++k) {
            MUST(out[1].E[k].layer_id == (uint32_t)(k % 3) && out[0].E[small.E.size() + k].layer_id == 5u + k % 3, "remapped ids");
            MUST(out[1].E[k].w.lo == flat.E[k].w.lo && out[0].E[small.E.size() + k].w.lo == flat.E[k].w.lo, "weights");
        }
        for (int k = 0; k < 3; ++k) MUST(same_layer(out[1].L[k], flat.L[at[k]], 0), "kept layer %d", k);
        MUST(eng.deep_route_counts()[0] == 3, "two more deep terms");
    }
    // ---- compact_edges + compact_layers: distinct cells come out sorted by (layer, idx, P before M)
    {
        const Cipher in = heap(nl, 20, true);
        Cipher c = in;
        pvac_hip::compact_edges(pk, c);
        MUST(c.L.size() == nl && c.E.size() == in.E.size(), "compact: %zu layers, %zu edges", c.L.size(), c.E.size());
        std::vector<Edge> want = in.E;
        std::stable_sort(want.begin(), want.end(), [](const Edge& a, const Edge& b) {
            return std::make_tuple(a.layer_id, a.idx, a.ch) < std::make_tuple(b.layer_id, b.idx, b.ch);
        });
        for (size_t e = 0; e < want.size(); ++e)
            MUST(same_edge(c.E[e], want[e], 0) && c.E[e].s.nbits == 8192 && c.E[e].s.w == want[e].s.w, "compact: edge %zu", e);
        for (uint32_t l = 0; l < nl; ++l) MUST(same_layer(c.L[l], in.L[l], 0), "compact: layer %u", l);
        MUST(eng.deep_route_counts()[2] == 1, "one deep cipher compacted");
    }
    // ---- ct_recrypt: zero sigma rows everywhere, so eight iterations; every sum is above 30,000 layers
    {
        mirror::EvalKey ek;
        ek.zero_pool = {heap(2, 3, true), heap(2, 4, true)};
        const Cipher in = heap(nl, 10, true);
        std::vector<uint32_t> iters;
        const auto out = pvac_hip::ct_recrypt_batch(pk, ek, std::vector<Cipher>{in}, [] { return (uint64_t)0; }, &iters);
        MUST(out.size() == 1 && iters.size() == 1 && iters[0] == 8, "ct_recrypt: %u iterations", iters.empty() ? 99u : iters[0]);
        MUST(out[0].L.size() == nl + 16 && out[0].E.size() == in.E.size() + 8 * ek.zero_pool[0].E.size(),
             "ct_recrypt: %zu layers, %zu edges", out[0].L.size(), out[0].E.size());
        for (uint32_t l = 0; l < nl; ++l) MUST(same_layer(out[0].L[l], in.L[l], 0), "ct_recrypt: layer %u", l);
        const auto n = eng.deep_route_counts();
        // the adapter draws lazily, one more word per pass: nine passes, each of eight sums and one compaction
        MUST(n[3] == 72 && n[2] == 1 + 9,"ct_recrypt: %llu deep sums, %llu deep compactions", (unsigned long long)n[3],
             (unsigned long long)n[2]);
    }
    // ---- another key's engine keeps the default limit: the same calls are refused as they always were
    {
        mirror::PubKey pk2 = pk;
        pk2.canon_tag = 0xD0D2;
        std::string what;
        try {
            (void)pvac_hip::ct_sum(pk2, std::vector<Cipher>{deep, small}, false);
        } catch (const pvac_hip::Error& e) {
            MUST(e.code == PVAC_ENOSYS, "ct_sum at the default limit: code %d", e.code);
            what = e.what();
        }
        MUST(what.find("ct_lincomb_plan: a term above 30000 layers") != std::string::npos, "message '%s'", what.c_str());
        const auto n = pvac_hip::engine_for(pk2).deep_route_counts();
        MUST(n[0] == 0 && n[1] == 0 && n[2] == 0 && n[3] == 0, "the default engine counted nothing");
    }
    std::printf("%d checks passed\n", g_checks);
    return 0;
}
