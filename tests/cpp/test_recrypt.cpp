// test_recrypt.cpp — ct_recrypt and its parts through the C++ adapter (include/pvac_hip.hpp), on types
// that mirror the reference's field layout (core/types.hpp:72-139), against the fixtures the
// unmodified reference minted (tests/golden/recrypt, tools/mint_recrypt.cpp). Runs on the GPU box:
//   test_recrypt <golden_dir> <canon_tag> <H_digest_hex> <name:d0,d1,...> ...
// one argument per fixture case with sigma: its name and the draws its iterations consumed.
// Exit 0 = every check passed; failures abort with a message.
#include <array>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <memory>
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
struct EvalKey { std::vector<Cipher> zero_pool; Cipher enc_one; };
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

// a .ct keeps BASE seeds and PROD parents only: project a full cipher the same way
static Cipher ct_view(Cipher c) {
    for (auto& L : c.L) {
        if (L.rule == mirror::RRule::PROD) L.seed = mirror::RSeed{};
        else { L.pa = 0; L.pb = 0; }
    }
    return c;
}

static std::vector<Cipher> read_ct(const std::string& path) { return pvac_hip::load_cts_bytes<Cipher>(slurp(path)); }
static std::vector<uint8_t> ct_bytes(const Cipher& c) { return pvac_hip::save_cts_bytes(std::vector<Cipher>{ct_view(c)}); }

struct replay {
    std::vector<uint64_t> s;
    size_t k = 0;
    uint64_t operator()() {
        MUST(k < s.size(), "random stream exhausted");
        return s[k++];
    }
};

static pvac_hip::RandomSource splitmix(uint64_t seed) {
    auto st = std::make_shared<uint64_t>(seed);
    return [st]() {
        uint64_t z = (*st += 0x9e3779b97f4a7c15ULL);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        return z ^ (z >> 31);
    };
}

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <golden_dir> <canon_tag> <H_digest_hex> <name:d0,d1,...> ...\n", argv[0]);
        return 2;
    }
    const std::string gold = argv[1], ref = gold + "/ref", rc = gold + "/recrypt";
    mirror::PubKey pk;
    pk.canon_tag = std::strtoull(argv[2], nullptr, 10);
    const std::string hdig = argv[3];
    for (int i = 0; i < 32; ++i) pk.H_digest[i] = (uint8_t)std::strtoul(hdig.substr(2 * i, 2).c_str(), nullptr, 16);
    {
        const auto b = slurp(rc + "/ubk_inv.i32");
        pk.ubk.inv.resize(b.size() / 4);
        std::memcpy(pk.ubk.inv.data(), b.data(), pk.ubk.inv.size() * 4);
        MUST(pk.ubk.inv.size() == 8192, "ubk_inv.i32");
    }
    const auto pg = [&] {
        const auto b = slurp(ref + "/powg_B.u64");
        std::vector<uint64_t> v(b.size() / 8);
        std::memcpy(v.data(), b.data(), v.size() * 8);
        return v;
    }();
    for (size_t i = 0; i + 1 < pg.size(); i += 2) pk.powg_B.push_back(mirror::Fp{pg[i], pg[i + 1]});
    mirror::SecKey sk;
    {
        const auto k = slurp(ref + "/sk_prf_k.u64");
        MUST(k.size() == 32, "sk_prf_k.u64");
        std::memcpy(sk.prf_k.data(), k.data(), 32);
        const auto s = slurp(ref + "/sk_lpn_s.u64");
        sk.lpn_s_bits.resize(s.size() / 8);
        std::memcpy(sk.lpn_s_bits.data(), s.data(), s.size());
    }
    mirror::EvalKey ek;
    ek.zero_pool = read_ct(rc + "/pool.ct");
    MUST(ek.zero_pool.size() == 4, "pool.ct");

    // ---- the reference's fixture cases through pvac_hip::ct_recrypt with a replaying source
    struct Case { std::string name; std::vector<uint64_t> draws; Cipher in; };
    std::vector<Case> cases;
    for (int a = 4; a < argc; ++a) {
        const std::string s = argv[a];
        const size_t c = s.find(':');
        MUST(c != std::string::npos, "case argument %s", s.c_str());
        Case k;
        k.name = s.substr(0, c);
        for (const char* p = s.c_str() + c + 1; *p;) {
            char* e = nullptr;
            k.draws.push_back(std::strtoull(p, &e, 10));
            p = *e ? e + 1 : e;
        }
        k.in = read_ct(rc + "/" + k.name + "_in.ct")[0];
        cases.push_back(k);
    }
    size_t most = 0;
    for (const Case& k : cases) {
        replay rs{k.draws};
        const Cipher out = pvac_hip::ct_recrypt(pk, ek, k.in, std::ref(rs));
        MUST(rs.k == k.draws.size(), "%s consumed %zu of %zu draws", k.name.c_str(), rs.k, k.draws.size());
        MUST(ct_bytes(out) == slurp(rc + "/" + k.name + "_out.ct"), "ct_recrypt %s .ct bytes", k.name.c_str());
        most = std::max(most, k.draws.size());
    }
    MUST(most == 8, "no fixture case reaches 8 iterations");
    {   // the batch form draws level by level, cipher order within a level
        std::vector<Cipher> in;
        replay rs;
        for (const Case& k : cases) in.push_back(k.in);
        for (size_t level = 0; level < 8; ++level)
            for (const Case& k : cases)
                if (k.draws.size() > level) rs.s.push_back(k.draws[level]);
        std::vector<uint32_t> iters;
        const std::vector<Cipher> out = pvac_hip::ct_recrypt_batch(pk, ek, in, std::ref(rs), &iters);
        MUST(rs.k == rs.s.size(), "batch consumed %zu of %zu draws", rs.k, rs.s.size());
        for (size_t i = 0; i < cases.size(); ++i) {
            MUST(iters[i] == cases[i].draws.size(), "batch iterations of %s", cases[i].name.c_str());
            MUST(ct_bytes(out[i]) == slurp(rc + "/" + cases[i].name + "_out.ct"), "batch %s", cases[i].name.c_str());
        }
    }
    {   // an empty pool and an empty cipher come back verbatim (recrypt.hpp:27)
        mirror::EvalKey none;
        const Cipher same = pvac_hip::ct_recrypt(pk, none, cases[0].in);
        MUST(ct_bytes(same) == ct_bytes(cases[0].in), "empty pool");
        Cipher empty;
        empty.L = cases[0].in.L;
        MUST(pvac_hip::ct_recrypt(pk, ek, empty).L.size() == empty.L.size(), "empty cipher");
    }

    // ---- the parts: sigma_density, ubk_apply, compact_edges
    for (const Case& k : cases) {
        long double ones = 0, total = 0;
        for (const auto& e : k.in.E) {
            for (uint64_t w : e.s.w) ones += __builtin_popcountll(w);
            total += pk.prm.m_bits;
        }
        MUST(pvac_hip::sigma_density(pk, k.in) == (double)(ones / total), "sigma_density %s", k.name.c_str());
    }
    {
        Cipher c = cases[0].in, want = cases[0].in;
        for (auto& e : want.E) {
            std::vector<uint64_t> o(e.s.w.size(), 0);
            for (size_t src = 0; src < 8192; ++src)
                if ((e.s.w[src >> 6] >> (src & 63)) & 1) {
                    const int j = pk.ubk.inv[src];
                    o[(size_t)j >> 6] |= 1ull << (j & 63);
                }
            e.s.w = o;
        }
        pvac_hip::ubk_apply(pk, c);
        MUST(ct_bytes(c) == ct_bytes(want), "ubk_apply");
    }
    for (const Case& k : cases)
        if (k.draws.empty()) {   // no iteration: the output is the compacted input
            Cipher c = k.in;
            pvac_hip::compact_edges(pk, c);
            MUST(ct_bytes(c) == slurp(rc + "/" + k.name + "_out.ct"), "compact_edges %s", k.name.c_str());
        }

    // ---- make_evalkey, and decryption through a recrypt (tests/test_main.cpp:285-287)
    {
        const mirror::EvalKey mk = pvac_hip::make_evalkey<mirror::EvalKey>(pk, sk, 3, 0, splitmix(0x5EED7001));
        MUST(mk.zero_pool.size() == 3, "make_evalkey pool size");
        for (const Cipher& z : mk.zero_pool) {
            const auto m = pvac_hip::dec_value(pk, sk, z);
            MUST(m.lo == 0 && m.hi == 0, "zero pool member decrypts to 0");
        }
        const auto one = pvac_hip::dec_value(pk, sk, mk.enc_one);
        MUST(one.lo == 1 && one.hi == 0, "enc_one decrypts to 1");
        const auto rnd = splitmix(0x5EED7002);
        const Cipher x = pvac_hip::enc_value<Cipher>(pk, sk, 1234567, rnd), y = pvac_hip::enc_value<Cipher>(pk, sk, 89, rnd);
        const Cipher p = pvac_hip::ct_mul(pk, x, y, rnd);
        const Cipher r = pvac_hip::ct_recrypt(pk, mk, p, rnd);
        const auto a = pvac_hip::dec_value(pk, sk, p), b = pvac_hip::dec_value(pk, sk, r);
        MUST(a.lo == 1234567ull * 89 && a.hi == 0 && b.lo == a.lo && b.hi == a.hi, "dec(ct_recrypt(x y)) == dec(x y)");
        // a skewed product iterates; the zero pool keeps the plaintext
        Cipher q = p;
        for (auto& e : q.E)
            for (auto& w : e.s.w) w &= (w << 1) | (w >> 63);
        const Cipher r2 = pvac_hip::ct_recrypt(pk, mk, q, rnd);
        MUST(r2.L.size() > p.L.size(), "a skewed product takes pool members");
        const auto c2 = pvac_hip::dec_value(pk, sk, r2);
        MUST(c2.lo == a.lo && c2.hi == 0, "dec(ct_recrypt(skewed x y)) == dec(x y)");
    }
    std::printf("%d checks passed\n", g_checks);
    return 0;
}
