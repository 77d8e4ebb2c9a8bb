// test_commit.cpp — commit_ct through the C++ adapter (include/pvac_hip.hpp), on types that mirror
// the reference's field layout (core/types.hpp:72-139), against the digests the unmodified reference
// minted for the fixture files. Runs on the GPU box:
//   test_commit <canon_tag> <H_digest_hex> <file.ct>:<0|1 with sigma>:<digest_hex> ...
// Exit 0 = every check passed; failures abort with a message.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
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

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <canon_tag> <H_digest_hex> <file.ct>:<0|1>:<digest_hex> ...\n", argv[0]);
        return 2;
    }
    mirror::PubKey pk;
    pk.canon_tag = std::strtoull(argv[1], nullptr, 10);
    const std::string hdig = argv[2];
    MUST(hdig.size() == 64, "H_digest");
    for (int i = 0; i < 32; ++i) pk.H_digest[i] = (uint8_t)std::strtoul(hdig.substr(2 * i, 2).c_str(), nullptr, 16);

    std::vector<Cipher> cs;
    std::vector<std::string> want, name;
    size_t with = 0, without = 0;
    for (int a = 3; a < argc; ++a) {
        const std::string s = argv[a];
        const size_t c2 = s.rfind(':'), c1 = c2 == std::string::npos || c2 == 0 ? std::string::npos : s.rfind(':', c2 - 1);
        MUST(c1 != std::string::npos, "argument %s", s.c_str());
        std::vector<Cipher> file = pvac_hip::load_cts_bytes<Cipher>(slurp(s.substr(0, c1)));
        MUST(file.size() == 1, "%s holds %zu ciphers", s.c_str(), file.size());
        const bool sig = s[c1 + 1] == '1';
        for (const auto& e : file[0].E) MUST(e.s.nbits == (sig ? 8192u : 0u), "%s: edge nbits %zu", s.c_str(), e.s.nbits);
        (sig ? with : without) += 1;
        cs.push_back(std::move(file[0]));
        want.push_back(s.substr(c2 + 1));
        name.push_back(s.substr(0, c1));
    }
    MUST(with && without, "the cases must mix ciphers with sigma and weights-only ones");

    // one at a time, then the whole mixed batch (two ABI calls inside)
    for (size_t i = 0; i < cs.size(); ++i)
        MUST(hex(pvac_hip::commit_ct(pk, cs[i])) == want[i], "commit_ct %s", name[i].c_str());
    const auto all = pvac_hip::commit_ct_batch(pk, cs);
    MUST(all.size() == cs.size(), "batch size");
    for (size_t i = 0; i < cs.size(); ++i) MUST(hex(all[i]) == want[i], "commit_ct_batch %s", name[i].c_str());
    MUST(pvac_hip::commit_ct_batch(pk, std::vector<Cipher>{}).empty(), "empty batch");

    // the with-sigma cipher stripped of its sigmas commits as its weights alone: differs from the full one
    {
        Cipher w = cs[0];
        for (auto& e : w.E) e.s = mirror::BitVec{};
        const auto d = pvac_hip::commit_ct(pk, w);
        MUST(w.E.empty() || hex(d) != want[0], "weights-only digest equals the with-sigma one");
    }
    // any other sigma width is refused, as the codec refuses mixed widths: no host fallback
    for (int kind = 0; kind < 2; ++kind) {
        Cipher bad;
        for (const Cipher& c : cs)
            if (c.E.size() >= 2 && c.E[0].s.nbits) bad = c;
        MUST(bad.E.size() >= 2, "no with-sigma cipher of two edges among the cases");
        if (kind == 0) bad.E[1].s = mirror::BitVec{};                    // edges disagree
        else for (auto& e : bad.E) { e.s.nbits = 4096; e.s.w.resize(64); }   // a width that is not m_bits
        bool threw = false;
        try { (void)pvac_hip::commit_ct(pk, bad); } catch (const pvac_hip::Error&) { threw = true; }
        MUST(threw, "sigma width kind %d not refused", kind);
    }
    std::printf("%d checks passed\n", g_checks);
    return 0;
}
