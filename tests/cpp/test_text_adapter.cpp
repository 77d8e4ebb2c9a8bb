// test_text_adapter.cpp — enc_text / dec_text / enc_fp_depth through the C++ adapter
// (include/pvac_hip.hpp) over libpvac_hip.so, with Cipher/PubKey types that mirror the reference's
// field layout (core/types.hpp:72-139), against the fixtures the unmodified reference minted
// (tests/golden/text, tools/mint_text.cpp). Runs on the GPU box; tests/test_cpp_text.py passes per case
//   <name>:<seed>:<draws>:<sigma 0|1>:<parts>:<msg hex or ->:<off,cnt,off,cnt,...>
// The replay source serves every cipher's logged draw segment padded with zeros to the words the
// adapter takes for that item (Engine::enc_items_draws). With PVAC_TEXT_DUMP=<dir> in the environment
// every message's ciphers are also written to <dir>/<name>.ct, for the caller to decrypt elsewhere.
#include <array>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
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
    double noise_entropy_bits = 120.0, tuple2_fraction = 0.55, depth_slope_bits = 16.0;
    size_t edge_budget = 1200000;
    int lpn_n = 4096, lpn_t = 16384, lpn_tau_num = 1, lpn_tau_den = 8;
};
struct Ubk { std::vector<int> perm; std::vector<int> inv; };
struct PubKey {
    Params prm; uint64_t canon_tag = 0; std::vector<BitVec> H; Ubk ubk;
    std::array<uint8_t, 32> H_digest{}; std::vector<Fp> powg_B;
};
struct SecKey { std::array<uint64_t, 4> prf_k{}; std::vector<uint64_t> lpn_s_bits; };
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

struct replay {
    std::vector<uint64_t> s;
    size_t k = 0;
    uint64_t operator()() {
        MUST(k < s.size(), "random stream exhausted");
        return s[k++];
    }
};

static std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out(1);
    for (char ch : s) {
        if (ch == sep) out.emplace_back();
        else out.back() += ch;
    }
    return out;
}

struct Case {
    std::string name, msg;
    bool sigma;
    int parts;
    std::vector<uint64_t> log;
    std::vector<std::pair<size_t, size_t>> seg;
};

using Item = pvac_hip::Engine::EncItem;

static std::vector<Item> text_items(const std::string& msg) {
    std::vector<Item> its{Item{PVAC_ENC_ITEM_VALUE, (uint64_t)msg.size(), 0, 0}};
    for (size_t b = 0; 15 * b < msg.size(); ++b) its.push_back(Item{PVAC_ENC_ITEM_FP, 0, 0, (int)(2 + b)});
    return its;
}

// the case's segments, each padded to the words the adapter takes for its item
static void append_stream(const mirror::PubKey& pk, const Case& k, std::vector<uint64_t>& s) {
    const std::vector<uint64_t> take = pvac_hip::engine_for(pk).enc_items_draws(pk, text_items(k.msg));
    MUST(take.size() == k.seg.size(), "%s: %zu items, %zu segments", k.name.c_str(), take.size(), k.seg.size());
    for (size_t i = 0; i < take.size(); ++i) {
        MUST(k.seg[i].second <= take[i], "%s: cipher %zu drew %zu words, the adapter takes %" PRIu64, k.name.c_str(), i,
             k.seg[i].second, take[i]);
        s.insert(s.end(), k.log.begin() + k.seg[i].first, k.log.begin() + k.seg[i].first + k.seg[i].second);
        s.insert(s.end(), (size_t)take[i] - k.seg[i].second, 0);
    }
}

static bool same_records(const Cipher& a, const Cipher& b) {
    if (a.L.size() != b.L.size() || a.E.size() != b.E.size()) return false;
    for (size_t i = 0; i < a.L.size(); ++i)
        if (a.L[i].rule != b.L[i].rule || a.L[i].seed.ztag != b.L[i].seed.ztag || a.L[i].seed.nonce.lo != b.L[i].seed.nonce.lo ||
            a.L[i].seed.nonce.hi != b.L[i].seed.nonce.hi)
            return false;
    for (size_t i = 0; i < a.E.size(); ++i)
        if (a.E[i].layer_id != b.E[i].layer_id || a.E[i].idx != b.E[i].idx || a.E[i].ch != b.E[i].ch ||
            a.E[i].w.lo != b.E[i].w.lo || a.E[i].w.hi != b.E[i].w.hi)
            return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <golden_dir> <canon_tag> <H_digest_hex> <case> ...\n", argv[0]);
        return 2;
    }
    const std::string gold = argv[1], ref = gold + "/ref", tx = gold + "/text";
    mirror::PubKey pk;
    pk.canon_tag = std::strtoull(argv[2], nullptr, 10);
    const std::string hdig = argv[3];
    for (int i = 0; i < 32; ++i) pk.H_digest[i] = (uint8_t)std::strtoul(hdig.substr(2 * i, 2).c_str(), nullptr, 16);
    {
        const auto b = slurp(ref + "/powg_B.u64");
        std::vector<uint64_t> v(b.size() / 8);
        std::memcpy(v.data(), b.data(), v.size() * 8);
        for (size_t i = 0; i + 1 < v.size(); i += 2) pk.powg_B.push_back(mirror::Fp{v[i], v[i + 1]});
    }
    mirror::SecKey sk;
    {
        const auto k = slurp(ref + "/sk_prf_k.u64");
        MUST(k.size() == 32, "sk_prf_k.u64");
        std::memcpy(sk.prf_k.data(), k.data(), 32);
        const auto s = slurp(ref + "/sk_lpn_s.u64");
        sk.lpn_s_bits.resize(s.size() / 8);
        std::memcpy(sk.lpn_s_bits.data(), s.data(), s.size());
    }

    std::vector<Case> cases;
    for (int a = 4; a < argc; ++a) {
        const std::vector<std::string> f = split(argv[a], ':');
        MUST(f.size() == 7, "case argument %s", argv[a]);
        Case k;
        k.name = f[0];
        uint64_t st = std::strtoull(f[1].c_str(), nullptr, 10);
        k.log.resize(std::strtoull(f[2].c_str(), nullptr, 10));
        for (uint64_t& w : k.log) {   // the mint tool's interposed getrandom: splitmix64 from the case's seed
            uint64_t z = (st += 0x9e3779b97f4a7c15ULL);
            z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
            z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
            w = z ^ (z >> 31);
        }
        k.sigma = f[3] == "1";
        k.parts = std::atoi(f[4].c_str());
        if (f[5] != "-")
            for (size_t i = 0; i + 1 < f[5].size(); i += 2) k.msg += (char)std::strtoul(f[5].substr(i, 2).c_str(), nullptr, 16);
        const std::vector<std::string> nums = split(f[6], ',');
        for (size_t i = 0; i + 1 < nums.size(); i += 2)
            k.seg.emplace_back((size_t)std::strtoull(nums[i].c_str(), nullptr, 10), (size_t)std::strtoull(nums[i + 1].c_str(), nullptr, 10));
        cases.push_back(k);
    }

    // ---- every message alone: the fixture's bytes (or records), and dec_text returns the message
    std::vector<std::vector<Cipher>> singles;
    std::vector<std::string> msgs;
    std::vector<uint64_t> all_stream;
    for (const Case& k : cases) {
        replay rs;
        append_stream(pk, k, rs.s);
        all_stream.insert(all_stream.end(), rs.s.begin(), rs.s.end());
        const std::vector<Cipher> out = pvac_hip::enc_text<Cipher>(pk, sk, k.msg, std::ref(rs));
        MUST(rs.k == rs.s.size(), "%s consumed %zu of %zu words", k.name.c_str(), rs.k, rs.s.size());
        MUST(out.size() == k.seg.size(), "%s: %zu ciphers", k.name.c_str(), out.size());
        if (k.sigma) {
            MUST(pvac_hip::save_cts_bytes(out) == slurp(tx + "/" + k.name + ".ct"), "%s: .ct bytes differ", k.name.c_str());
        } else {
            std::vector<Cipher> want;
            for (int p = 0; p < k.parts; ++p) {
                const auto part = pvac_hip::load_cts_bytes<Cipher>(slurp(tx + "/" + k.name + "_p" + std::to_string(p) + ".ct"));
                want.insert(want.end(), part.begin(), part.end());
            }
            MUST(want.size() == out.size(), "%s: parts hold %zu ciphers", k.name.c_str(), want.size());
            for (size_t i = 0; i < out.size(); ++i) MUST(same_records(out[i], want[i]), "%s: cipher %zu differs", k.name.c_str(), i);
        }
        MUST(pvac_hip::dec_text(pk, sk, out) == k.msg, "%s: dec_text", k.name.c_str());
        if (const char* dump = std::getenv("PVAC_TEXT_DUMP")) {
            const std::vector<uint8_t> b = pvac_hip::save_cts_bytes(out);
            std::ofstream o(std::string(dump) + "/" + k.name + ".ct", std::ios::binary);
            o.write((const char*)b.data(), (std::streamsize)b.size());
            MUST(o.good(), "write %s/%s.ct", dump, k.name.c_str());
        }
        singles.push_back(out);
        msgs.push_back(k.msg);
    }
    // ---- all of them in one batch, from the same words
    {
        replay rs{all_stream};
        const auto batch = pvac_hip::enc_text_batch<Cipher>(pk, sk, msgs, true, std::ref(rs));
        MUST(rs.k == rs.s.size() && batch.size() == msgs.size(), "batch: %zu of %zu words", rs.k, rs.s.size());
        for (size_t m = 0; m < msgs.size(); ++m)
            MUST(pvac_hip::save_cts_bytes(batch[m]) == pvac_hip::save_cts_bytes(singles[m]), "batch: message %zu differs", m);
        MUST(pvac_hip::dec_text_batch(pk, sk, batch) == msgs, "dec_text_batch");
    }
    // ---- a bare enc_fp_depth decrypts to its plaintext; no layer is added
    {
        const mirror::Fp v{0x0123456789ABCDEFULL, 0x00FEDCBA98765432ULL};
        const Cipher c = pvac_hip::enc_fp_depth<Cipher>(pk, sk, v, 5);
        MUST(c.L.size() == 1, "enc_fp_depth: %zu layers", c.L.size());
        const mirror::Fp d = pvac_hip::dec_value(pk, sk, c);
        MUST(d.lo == v.lo && d.hi == v.hi, "enc_fp_depth: decrypts to %016" PRIx64 "%016" PRIx64, d.hi, d.lo);
    }
    // ---- 124 blocks need depth hint 125: refused before any draw
    {
        replay none;
        int code = 0;
        try {
            (void)pvac_hip::enc_text<Cipher>(pk, sk, std::string(1846, 'x'), std::ref(none));
        } catch (const pvac_hip::Error& e) {
            code = e.code;
        }
        MUST(code == PVAC_ENOSYS && none.k == 0, "1846 bytes: code %d", code);
        MUST(pvac_hip::dec_text(pk, sk, pvac_hip::enc_text<Cipher>(pk, sk, std::string(47, 'y'))) == std::string(47, 'y'),
             "roundtrip on OS randomness");
        MUST(pvac_hip::dec_text(pk, sk, std::vector<Cipher>{}).empty(), "dec_text of no ciphers");
    }
    std::printf("%d checks passed\n", g_checks);
    return 0;
}
