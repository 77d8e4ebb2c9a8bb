// test_text_wide_adapter.cpp — the C++ adapter (include/pvac_hip.hpp) above 256 pre-merge edges per half:
// with engine_for(pk).set_enc_plan_limit raised, enc_text, enc_fp_depth and make_evalkey run plans the
// default limit refuses, against the fixtures the unmodified reference minted (tests/golden/text_wide,
// tools/mint_text_wide.cpp). Runs on the GPU box; tests/test_cpp_text_wide.py passes
//   <golden_dir> <canon_tag> <H_digest_hex>
//   <name>:<seed>:<draws>:0:<parts>:<msg hex>:<off,cnt,...>:<commit,commit,...>     the text case
//   <seed>:<draws>:<off>:<cnt>:<hint>:<v_lo>:<v_hi>:<index in fpwide>:<parts>        one enc_fp_depth of fpwide
// The replay source serves every cipher's logged draw segment padded with zeros to the words the adapter
// takes for that item.
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
    std::vector<std::string> commits;
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

static std::vector<uint64_t> splitmix_log(uint64_t st, size_t n) {   // the mint tool's interposed getrandom
    std::vector<uint64_t> log(n);
    for (uint64_t& w : log) {
        uint64_t z = (st += 0x9e3779b97f4a7c15ULL);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        w = z ^ (z >> 31);
    }
    return log;
}

static std::string hex32(const std::array<uint8_t, 32>& d) {
    static const char* H = "0123456789abcdef";
    std::string s;
    for (uint8_t b : d) { s += H[b >> 4]; s += H[b & 15]; }
    return s;
}

static std::vector<Cipher> load_parts(const std::string& dir, const std::string& name, int parts) {
    std::vector<Cipher> want;
    for (int p = 0; p < parts; ++p) {
        const auto part = pvac_hip::load_cts_bytes<Cipher>(slurp(dir + "/" + name + "_p" + std::to_string(p) + ".ct"));
        want.insert(want.end(), part.begin(), part.end());
    }
    return want;
}

namespace mirror {
struct EvalKey { std::vector<Cipher> zero_pool; Cipher enc_one; };
}  // namespace mirror

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s <golden_dir> <canon_tag> <H_digest_hex> <text case> <fp item>\n", argv[0]);
        return 2;
    }
    const std::string gold = argv[1], ref = gold + "/ref", tx = gold + "/text_wide";
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
    Case k;
    {
        const std::vector<std::string> f = split(argv[4], ':');
        MUST(f.size() == 8, "case argument %s", argv[4]);
        k.name = f[0];
        k.log = splitmix_log(std::strtoull(f[1].c_str(), nullptr, 10), std::strtoull(f[2].c_str(), nullptr, 10));
        k.sigma = false;
        k.parts = std::atoi(f[4].c_str());
        for (size_t i = 0; i + 1 < f[5].size(); i += 2) k.msg += (char)std::strtoul(f[5].substr(i, 2).c_str(), nullptr, 16);
        const std::vector<std::string> nums = split(f[6], ',');
        for (size_t i = 0; i + 1 < nums.size(); i += 2)
            k.seg.emplace_back((size_t)std::strtoull(nums[i].c_str(), nullptr, 10), (size_t)std::strtoull(nums[i + 1].c_str(), nullptr, 10));
        k.commits = split(f[7], ',');
    }

    // ---- at the default limit the message is refused before any draw, as it always was
    pvac_hip::Engine& eng = pvac_hip::engine_for(pk);
    MUST(eng.enc_plan_limit() == PVAC_ENC_PLAN_LIMIT_DEFAULT, "default limit %u", eng.enc_plan_limit());
    {
        replay none;
        int code = 0;
        try {
            (void)pvac_hip::enc_text<Cipher>(pk, sk, k.msg, std::ref(none));
        } catch (const pvac_hip::Error& e) {
            code = e.code;
        }
        MUST(code == PVAC_ENOSYS && none.k == 0, "%zu bytes at the default limit: code %d", k.msg.size(), code);
    }
    eng.set_enc_plan_limit(512);
    MUST(eng.enc_plan_limit() == 512, "limit %u", eng.enc_plan_limit());

    // ---- enc_text of the message from its logged draws: the fixture's records and every commit with sigma
    {
        replay rs;
        append_stream(pk, k, rs.s);
        const std::vector<Cipher> out = pvac_hip::enc_text<Cipher>(pk, sk, k.msg, std::ref(rs));
        MUST(rs.k == rs.s.size(), "%s consumed %zu of %zu words", k.name.c_str(), rs.k, rs.s.size());
        MUST(out.size() == k.seg.size() && out.size() == k.commits.size(), "%s: %zu ciphers", k.name.c_str(), out.size());
        MUST(out.back().E.size() > 0 && k.seg.size() == 126, "%s: 126 ciphers, the last two wide", k.name.c_str());
        const std::vector<Cipher> want = load_parts(tx, k.name, k.parts);
        MUST(want.size() == out.size(), "%s: parts hold %zu ciphers", k.name.c_str(), want.size());
        const auto commits = pvac_hip::commit_ct_batch(pk, out);
        for (size_t i = 0; i < out.size(); ++i) {
            MUST(same_records(out[i], want[i]), "%s: cipher %zu differs", k.name.c_str(), i);
            MUST(hex32(commits[i]) == k.commits[i], "%s: commit %zu differs", k.name.c_str(), i);
        }
        MUST(pvac_hip::dec_text(pk, sk, out) == k.msg, "%s: dec_text", k.name.c_str());
    }
    // ---- enc_fp_depth at a wide hint from its logged draws
    {
        const std::vector<std::string> f = split(argv[5], ':');
        MUST(f.size() == 9, "fp argument %s", argv[5]);
        const std::vector<uint64_t> log = splitmix_log(std::strtoull(f[0].c_str(), nullptr, 10), std::strtoull(f[1].c_str(), nullptr, 10));
        const size_t off = std::strtoull(f[2].c_str(), nullptr, 10), cnt = std::strtoull(f[3].c_str(), nullptr, 10);
        const int hint = std::atoi(f[4].c_str());
        const mirror::Fp v{std::strtoull(f[5].c_str(), nullptr, 10), std::strtoull(f[6].c_str(), nullptr, 10)};
        eng.set_enc_plan_limit(PVAC_ENC_PLAN_LIMIT_DEFAULT);
        int code = 0;
        try {
            (void)pvac_hip::enc_fp_depth<Cipher>(pk, sk, v, hint);
        } catch (const pvac_hip::Error& e) {
            code = e.code;
        }
        MUST(code == PVAC_ENOSYS, "enc_fp_depth at hint %d and the default limit: code %d", hint, code);
        eng.set_enc_plan_limit(512);
        const std::vector<uint64_t> take = eng.enc_items_draws(pk, {Item{PVAC_ENC_ITEM_FP, v.lo, v.hi, hint}});
        MUST(take.size() == 1 && cnt <= take[0], "hint %d drew %zu words, the adapter takes %" PRIu64, hint, cnt, take[0]);
        replay rs;
        rs.s.assign(log.begin() + off, log.begin() + off + cnt);
        rs.s.insert(rs.s.end(), (size_t)take[0] - cnt, 0);
        const Cipher c = pvac_hip::enc_fp_depth<Cipher>(pk, sk, v, hint, std::ref(rs));
        const std::vector<Cipher> want = load_parts(tx, "fpwide", std::atoi(f[8].c_str()));
        const size_t at = std::strtoull(f[7].c_str(), nullptr, 10);
        MUST(at < want.size() && same_records(c, want[at]), "enc_fp_depth at hint %d differs from fpwide[%zu]", hint, at);
        MUST(c.L.size() == 1 && c.E.size() > 256, "hint %d: %zu layers, %zu edges", hint, c.L.size(), c.E.size());
    }
    // ---- a recrypt pool minted for a depth above 124: every pool cipher decrypts to 0, enc_one to 1
    {
        const mirror::EvalKey ek = pvac_hip::make_evalkey<mirror::EvalKey>(pk, sk, 3, 125);
        MUST(ek.zero_pool.size() == 3, "pool of %zu", ek.zero_pool.size());
        for (const Cipher& z : ek.zero_pool) {
            MUST(z.L.size() == 2 && z.E.size() > 256, "pool cipher: %zu layers, %zu edges", z.L.size(), z.E.size());
            const mirror::Fp d = pvac_hip::dec_value(pk, sk, z);
            MUST(d.lo == 0 && d.hi == 0, "pool cipher decrypts to %016" PRIx64 "%016" PRIx64, d.hi, d.lo);
        }
        const mirror::Fp one = pvac_hip::dec_value(pk, sk, ek.enc_one);
        MUST(one.lo == 1 && one.hi == 0, "enc_one");
    }
    std::printf("%d checks passed\n", g_checks);
    return 0;
}
