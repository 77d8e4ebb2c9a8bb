// test_metrics.cpp — the metrics of utils/metrics.hpp through the C++ adapter (include/pvac_hip.hpp), on
// types that mirror the reference's field layout (core/types.hpp:72-139), on two hand-built ciphers
// with sigma. Runs on the GPU box, in a scratch working directory (it appends to pvac_metrics.csv):
//   test_metrics
// Exit 0 = every check passed; failures abort with a message.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
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
    int B = 337, m_bits = 8192, n_bits = 16384, h_col_wt = 192, x_col_wt = 128, err_wt = 128;
    size_t edge_budget = 1200000;
};
struct PubKey { Params prm; uint64_t canon_tag = 0; std::array<uint8_t, 32> H_digest{}; std::vector<Fp> powg_B; };
}  // namespace mirror

using mirror::Cipher;
using mirror::Fp;

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

static uint64_t mix(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

// the test's own entropy loop over the test's own counts
static double shannon(const Cipher& c) {
    std::array<uint64_t, 256> freq{};
    uint64_t total = 0;
    for (const auto& e : c.E)
        for (uint64_t w : e.s.w)
            for (int k = 0; k < 8; ++k) {
                ++freq[(w >> (8 * k)) & 0xFF];
                ++total;
            }
    if (!total) return 0.0;
    double H = 0.0;
    for (int b = 0; b < 256; ++b)
        if (freq[b] > 0) {
            const double p = (double)freq[b] / total;
            H -= p * std::log2(p);
        }
    return H;
}

static Cipher make(uint64_t seed, uint32_t layers, const std::vector<std::array<uint32_t, 4>>& edges, int sigma_kind) {
    Cipher c;
    for (uint32_t l = 0; l < layers; ++l) c.L.push_back({mirror::RRule::BASE, {mix(seed), {mix(seed), mix(seed)}}, 0, 0});
    for (const auto& e : edges) {   // {layer, idx, ch, small weight}
        mirror::Edge x{e[0], (uint16_t)e[1], (uint8_t)e[2], Fp{e[3], 0}, {}};
        x.s.nbits = 8192;
        x.s.w.resize(128);
        for (auto& w : x.s.w) w = sigma_kind == 0 ? mix(seed) : sigma_kind == 1 ? 0 : (mix(seed) & 0x0101010101010101ULL);
        c.E.push_back(std::move(x));
    }
    return c;
}

int main() {
    // powg_B[i] = i + 1: every term w * powg_B[idx] is a small integer, so the expected sums below are
    // plain arithmetic, negative ones written as p - k with p = 2^127 - 1
    mirror::PubKey pk;
    pk.canon_tag = 0x4D45;
    for (int i = 0; i < pk.prm.B; ++i) pk.powg_B.push_back(Fp{(uint64_t)i + 1, 0});
    const uint64_t P_LO = ~0ULL, P_HI = 0x7FFFFFFFFFFFFFFFULL;

    // a: layer 0 = +5*1 + 7*11 - 3*4 = 70; layer 1 = -(2*337) = p - 674; layer 2 has no edge = 0
    const Cipher a = make(1, 3, {{0, 0, 0, 5}, {0, 10, 0, 7}, {0, 3, 1, 3}, {1, 336, 1, 2}}, 0);
    // b: layer 0 = 9*2 - 9*2 = 0; layer 1 = +1*1 = 1; its sigma bytes are 0 or 1 only
    const Cipher b = make(2, 2, {{0, 1, 0, 9}, {0, 1, 1, 9}, {1, 0, 0, 1}}, 2);
    const Cipher z = make(3, 1, {{0, 0, 0, 1}}, 1);   // all-zero sigma: entropy 0
    const Cipher empty;
    Cipher bare = a;                                   // no sigma words at all: the reference's total == 0
    for (auto& e : bare.E) e.s = mirror::BitVec{};

    // sigma_shannon: bit for bit the restated loop
    const std::vector<Cipher> cs = {a, b, z, empty, bare};
    for (const Cipher& c : cs) {
        const double got = pvac_hip::sigma_shannon(pk, c), want = shannon(c);
        MUST(std::memcmp(&got, &want, sizeof got) == 0, "sigma_shannon %.17g != %.17g", got, want);
    }
    const std::vector<double> all = pvac_hip::sigma_shannon_batch(pk, cs);
    MUST(all.size() == cs.size(), "batch size");
    for (size_t i = 0; i < cs.size(); ++i) {
        const double want = shannon(cs[i]);
        MUST(std::memcmp(&all[i], &want, sizeof want) == 0, "sigma_shannon_batch[%zu] %.17g != %.17g", i, all[i], want);
    }
    MUST(shannon(a) > 7.9 && shannon(a) <= 8.0 && shannon(z) == 0.0 && all[3] == 0.0 && all[4] == 0.0, "the cases' entropies");
    MUST(shannon(b) > 0.9 && shannon(b) <= 1.0, "two byte values: about one bit");

    // agg_layer_gsum against the tables above
    const Fp wa[3] = {{70, 0}, {P_LO - 674, P_HI}, {0, 0}}, wb[2] = {{0, 0}, {1, 0}};
    for (uint32_t l = 0; l < 3; ++l) {
        const Fp g = pvac_hip::agg_layer_gsum<Fp>(pk, a, l);
        MUST(g.lo == wa[l].lo && g.hi == wa[l].hi, "agg_layer_gsum(a, %u) = (%llx, %llx)", l, (unsigned long long)g.lo,
             (unsigned long long)g.hi);
    }
    const Fp past = pvac_hip::agg_layer_gsum<Fp>(pk, a, 7);
    MUST(past.lo == 0 && past.hi == 0, "a layer id past |L| sums nothing");
    const auto gs = pvac_hip::layer_gsums_batch<Fp>(pk, std::vector<Cipher>{a, empty, b});
    MUST(gs.size() == 3 && gs[0].size() == 3 && gs[1].empty() && gs[2].size() == 2, "layer_gsums_batch shape");
    for (uint32_t l = 0; l < 3; ++l) MUST(gs[0][l].lo == wa[l].lo && gs[0][l].hi == wa[l].hi, "batch a layer %u", l);
    for (uint32_t l = 0; l < 2; ++l) MUST(gs[2][l].lo == wb[l].lo && gs[2][l].hi == wb[l].hi, "batch b layer %u", l);

    // dump_metrics: header then row, appended to pvac_metrics.csv of the working directory
    {
        std::ifstream before("pvac_metrics.csv");
        MUST(!before.good(), "run in a scratch directory: pvac_metrics.csv exists");
    }
    pvac_hip::dump_metrics(pk, "step1", z, Fp{42, 7});
    pvac_hip::dump_metrics(pk, "step2", empty, Fp{0, 0});
    std::ifstream f("pvac_metrics.csv");
    std::stringstream got;
    got << f.rdbuf();
    const std::string want =
        "tag,edges,layers,sigma_density,value_lo,value_hi\n"
        "step1,1,1,0.000000,42,7\n"
        "step2,0,0,0.000000,0,0\n";
    MUST(got.str() == want, "pvac_metrics.csv holds:\n%s", got.str().c_str());
    // a density that is not zero, six fixed decimals: a's first edge alone, all ones but 64 bits
    {
        Cipher d = make(5, 1, {{0, 0, 0, 1}}, 1);
        for (auto& w : d.E[0].s.w) w = ~0ULL;
        d.E[0].s.w[5] = 0;
        pvac_hip::dump_metrics(pk, "step3", d, Fp{1, 2});
        std::ifstream f2("pvac_metrics.csv");
        std::stringstream g2;
        g2 << f2.rdbuf();
        MUST(g2.str() == want + "step3,1,1,0.992188,1,2\n", "pvac_metrics.csv holds:\n%s", g2.str().c_str());
    }
    std::printf("%d checks passed\n", g_checks);
    return 0;
}
