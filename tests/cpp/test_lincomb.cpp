// test_lincomb.cpp — ct_sum / ct_lincomb / ct_lincomb_batch through the C++ adapter
// (include/pvac_hip.hpp), on types that mirror the reference's field layout (core/types.hpp:72-139),
// against the digests the unmodified reference minted for tests/golden/lincomb. Runs on the GPU box:
//   test_lincomb <canon_tag> <H_digest_hex> <edge_budget> <golden dir> <case file>
// The case file (written by tests/test_cpp_lincomb.py from the manifest) holds, per case, a line
//   <name> <sigma 0|1> <commit hex> <n_terms>
// and per term a line <path under golden> <flag> <scale lo> <scale hi>. Every case of one run shares
// the edge budget (one engine per public key). Exit 0 = every check passed.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
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
struct PubKey { Params prm; uint64_t canon_tag = 0; std::array<uint8_t, 32> H_digest{}; };
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

static std::vector<uint8_t> slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    MUST(f.good(), "open %s", p.c_str());
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static std::string hex(const std::array<uint8_t, 32>& d) {
    char s[65];
    for (int i = 0; i < 32; ++i) std::snprintf(s + 2 * i, 3, "%02x", d[i]);
    return s;
}

struct Case {
    std::string name, commit;
    bool sigma = false;
    std::vector<std::string> path;
    std::vector<uint32_t> flags;
    std::vector<Fp> scales;
};

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s <canon_tag> <H_digest_hex> <edge_budget> <golden dir> <case file>\n", argv[0]);
        return 2;
    }
    mirror::PubKey pk;
    pk.canon_tag = std::strtoull(argv[1], nullptr, 10);
    const std::string hdig = argv[2], golden = argv[4];
    MUST(hdig.size() == 64, "H_digest");
    for (int i = 0; i < 32; ++i) pk.H_digest[i] = (uint8_t)std::strtoul(hdig.substr(2 * i, 2).c_str(), nullptr, 16);
    pk.prm.edge_budget = std::strtoull(argv[3], nullptr, 10);

    std::vector<Case> cases;
    {
        std::ifstream f(argv[5]);
        MUST(f.good(), "open %s", argv[5]);
        Case c;
        int sig = 0;
        size_t m = 0;
        while (f >> c.name >> sig >> c.commit >> m) {
            c.sigma = sig != 0;
            c.path.assign(m, "");
            c.flags.assign(m, 0);
            c.scales.assign(m, Fp{0, 0});
            for (size_t k = 0; k < m; ++k) MUST(bool(f >> c.path[k] >> c.flags[k] >> c.scales[k].lo >> c.scales[k].hi), "case file");
            cases.push_back(c);
        }
    }
    MUST(!cases.empty(), "no cases");

    std::map<std::string, Cipher> files;
    auto load = [&](const std::string& p, bool sigma) {
        if (!files.count(p)) {
            std::vector<Cipher> file = pvac_hip::load_cts_bytes<Cipher>(slurp(golden + "/" + p));
            MUST(!file.empty(), "%s holds no cipher", p.c_str());
            files[p] = file[0];
        }
        Cipher c = files[p];
        if (!sigma)
            for (auto& e : c.E) e.s = mirror::BitVec{};
        return c;
    };

    for (const Case& k : cases) {
        std::vector<Cipher> xs;
        std::vector<uint64_t> term;
        bool any = false, all = true;
        for (size_t j = 0; j < k.path.size(); ++j) {
            xs.push_back(load(k.path[j], k.sigma));
            term.push_back(j);
            any = any || (k.flags[j] & PVAC_TERM_SCALE);
            all = all && (k.flags[j] & PVAC_TERM_SCALE);
        }
        const std::vector<uint64_t> seg_off{0, (uint64_t)xs.size()};
        // the batch form with the case's own flags (no scales at all where nothing is flagged)
        const auto out = any ? pvac_hip::ct_lincomb_batch(pk, xs, seg_off, term, k.scales, k.flags, k.sigma)
                             : pvac_hip::ct_lincomb_batch(pk, xs, seg_off, term, std::vector<Fp>{}, {}, k.sigma);
        MUST(out.size() == 1, "%s: outputs", k.name.c_str());
        MUST(hex(pvac_hip::commit_ct(pk, out[0])) == k.commit, "ct_lincomb_batch %s", k.name.c_str());
        if (!any) MUST(hex(pvac_hip::commit_ct(pk, pvac_hip::ct_sum(pk, xs, k.sigma))) == k.commit, "ct_sum %s", k.name.c_str());
        if (all && !xs.empty())
            MUST(hex(pvac_hip::commit_ct(pk, pvac_hip::ct_lincomb(pk, xs, k.scales, k.sigma))) == k.commit, "ct_lincomb %s",
                 k.name.c_str());
    }
    // the weights-only cases as the segments of one call over a shared pool
    {
        std::vector<Cipher> pool;
        std::vector<uint64_t> seg_off{0}, term;
        std::vector<uint32_t> flags;
        std::vector<Fp> scales;
        std::vector<std::string> want;
        for (const Case& k : cases) {
            if (k.sigma) continue;
            for (size_t j = 0; j < k.path.size(); ++j) {
                term.push_back(pool.size());
                pool.push_back(load(k.path[j], false));
                flags.push_back(k.flags[j]);
                scales.push_back(k.scales[j]);
            }
            seg_off.push_back(term.size());
            want.push_back(k.commit);
        }
        if (!want.empty()) {
            const auto out = pvac_hip::ct_lincomb_batch(pk, pool, seg_off, term, scales, flags, false);
            MUST(out.size() == want.size(), "batch size");
            const auto dig = pvac_hip::commit_ct_batch(pk, out);
            for (size_t i = 0; i < want.size(); ++i) MUST(hex(dig[i]) == want[i], "segment %zu of the shared call", i);
        }
    }
    // a list that does not describe a call is refused on the host
    {
        bool threw = false;
        try {
            (void)pvac_hip::ct_lincomb_batch(pk, std::vector<Cipher>(2), {0, 2}, {0, 2}, std::vector<Fp>{});
        } catch (const pvac_hip::Error& e) { threw = e.code == PVAC_EINVAL; }
        MUST(threw, "a term index beyond the pool was not refused");
    }
    std::printf("%d checks passed\n", g_checks);
    return 0;
}
