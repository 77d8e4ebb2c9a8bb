// test_drbg.cpp — the C++ adapter's device_random forms on the GPU (include/pvac_hip.hpp): ct_mul_batch and
// enc_value_batch with every nonce, salt and draw filled by the context's CTR_DRBG (pvac_hip_drbg_fill),
// and the RandomSource forms beside them unchanged: a replayed reference stream still gives the
// reference's bytes. Built by tests/cpp/drbg.mk, run by tests/test_cpp_drbg.py:
//   test_drbg <golden_dir> <canon_tag> <H_digest_hex> <v0>
//   test_drbg --time <pairs>   ct_mul_batch (weights only) on the same host ciphers with os_random_u64 and
//                              with device_random, alternated: one JSON line with both rates (tools/exp_drbg.py)
#include <algorithm>
#include <array>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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
struct PubKey {
    Params prm; uint64_t canon_tag = 0; std::vector<BitVec> H;
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

// ---- .ct codec (format of the reference's tests/add.cpp:22-155; our own reader/writer)
static std::vector<uint8_t> slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    MUST(f.good(), "open %s", p.c_str());
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct reader {
    const std::vector<uint8_t>& b;
    size_t o = 0;
    template <class T> T get() {
        T v;
        MUST(o + sizeof(T) <= b.size(), "truncated .ct");
        std::memcpy(&v, &b[o], sizeof(T));
        o += sizeof(T);
        return v;
    }
};

static std::vector<Cipher> read_ct(const std::string& path) {
    const auto buf = slurp(path);
    reader r{buf};
    MUST(r.get<uint32_t>() == 0x66699666u && r.get<uint32_t>() == 1u, "bad .ct header %s", path.c_str());
    const uint64_t n = r.get<uint64_t>();
    std::vector<Cipher> out(n);
    for (auto& c : out) {
        const uint32_t nL = r.get<uint32_t>(), nE = r.get<uint32_t>();
        c.L.resize(nL);
        for (auto& L : c.L) {
            L = mirror::Layer{};
            L.rule = (mirror::RRule)r.get<uint8_t>();
            if (L.rule == mirror::RRule::BASE) {
                L.seed.ztag = r.get<uint64_t>();
                L.seed.nonce.lo = r.get<uint64_t>();
                L.seed.nonce.hi = r.get<uint64_t>();
            } else if (L.rule == mirror::RRule::PROD) {
                L.pa = r.get<uint32_t>();
                L.pb = r.get<uint32_t>();
            } else {
                r.o += 24;
            }
        }
        c.E.resize(nE);
        for (auto& E : c.E) {
            E.layer_id = r.get<uint32_t>();
            E.idx = r.get<uint16_t>();
            E.ch = r.get<uint8_t>();
            (void)r.get<uint8_t>();
            E.w.lo = r.get<uint64_t>();
            E.w.hi = r.get<uint64_t>();
            E.s.nbits = r.get<uint32_t>();
            E.s.w.resize((E.s.nbits + 63) / 64);
            for (auto& w : E.s.w) w = r.get<uint64_t>();
        }
    }
    MUST(r.o == buf.size(), "trailing bytes in %s", path.c_str());
    return out;
}

template <class T>
static void put(std::vector<uint8_t>& o, T v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    o.insert(o.end(), p, p + sizeof(T));
}

static std::vector<uint8_t> write_ct(const std::vector<Cipher>& cs) {
    std::vector<uint8_t> o;
    put<uint32_t>(o, 0x66699666u);
    put<uint32_t>(o, 1u);
    put<uint64_t>(o, cs.size());
    for (const auto& c : cs) {
        put<uint32_t>(o, (uint32_t)c.L.size());
        put<uint32_t>(o, (uint32_t)c.E.size());
        for (const auto& L : c.L) {
            put<uint8_t>(o, (uint8_t)L.rule);
            if (L.rule == mirror::RRule::BASE) {
                put(o, L.seed.ztag); put(o, L.seed.nonce.lo); put(o, L.seed.nonce.hi);
            } else {
                put(o, L.pa); put(o, L.pb);
            }
        }
        for (const auto& E : c.E) {
            put(o, E.layer_id); put(o, E.idx); put(o, E.ch); put<uint8_t>(o, 0);
            put(o, E.w.lo); put(o, E.w.hi);
            put<uint32_t>(o, (uint32_t)E.s.nbits);
            for (uint64_t w : E.s.w) put(o, w);
        }
    }
    return o;
}

static std::vector<uint64_t> read_u64(const std::string& p) {
    const auto b = slurp(p);
    std::vector<uint64_t> v(b.size() / 8);
    std::memcpy(v.data(), b.data(), v.size() * 8);
    return v;
}

// A .ct keeps BASE seeds and PROD parents only: project a full cipher the same way.
static Cipher ct_view(Cipher c) {
    for (auto& L : c.L) {
        if (L.rule == mirror::RRule::PROD) L.seed = mirror::RSeed{};
        else { L.pa = 0; L.pb = 0; }
    }
    return c;
}

static bool same_edges(const Cipher& a, const Cipher& b, bool sigma) {
    if (a.E.size() != b.E.size()) return false;
    for (size_t i = 0; i < a.E.size(); ++i) {
        const auto &x = a.E[i], &y = b.E[i];
        if (x.layer_id != y.layer_id || x.idx != y.idx || x.ch != y.ch || x.w.lo != y.w.lo || x.w.hi != y.w.hi)
            return false;
        if (sigma && x.s.w != y.s.w) return false;
    }
    return true;
}

// replays a reference random stream (nonces, then salts) like the harness' getrandom log
struct replay {
    std::vector<uint64_t> s;
    size_t k = 0;
    uint64_t operator()() {
        MUST(k < s.size(), "random stream exhausted");
        return s[k++];
    }
};

// reads past an enc_value log return 0 (the adapter draws a whole stride per value)
struct replay_pad {
    std::vector<uint64_t> s;
    size_t k = 0;
    uint64_t operator()() { return k < s.size() ? s[k++] : (++k, 0ull); }
};

// --time <pairs>: the by-value batched ct_mul (weights only) on host ciphers shaped like enc_value output
// (2 BASE layers x 20 distinct (idx, ch) edges), host ciphers in and out, with the nonces drawn by
// os_random_u64 (one getrandom per word, staged and uploaded) and by device_random, three rounds alternated
static int time_sources(size_t n) {
    uint64_t st = 0x5EED0016;
    auto rnd = [&]() {
        uint64_t z = (st += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    auto fresh = [&]() {
        Cipher c;
        c.L.resize(2);
        for (auto& l : c.L) { l.rule = mirror::RRule::BASE; l.seed.ztag = rnd(); l.seed.nonce = {rnd(), rnd()}; l.pa = l.pb = 0; }
        for (uint32_t la = 0; la < 2; ++la) {
            std::vector<uint32_t> used;
            while (used.size() < 20) {
                const uint32_t k = (uint32_t)(rnd() % (2 * 337));
                if (std::find(used.begin(), used.end(), k) != used.end()) continue;
                used.push_back(k);
                mirror::Edge e{};
                e.layer_id = la; e.idx = (uint16_t)(k >> 1); e.ch = (uint8_t)(k & 1);
                e.w = mirror::Fp{rnd(), rnd() & 0x7FFFFFFFFFFFFFFFull};
                c.E.push_back(e);
            }
        }
        return c;
    };
    std::vector<Cipher> A(n), B(n);
    for (size_t i = 0; i < n; ++i) { A[i] = fresh(); B[i] = fresh(); }
    mirror::PubKey pk;
    pk.canon_tag = 0x5EED0016;
    (void)pvac_hip::ct_mul_batch(pk, A, B, false, pvac_hip::os_random_u64);   // warm-up (allocations, code objects)
    (void)pvac_hip::ct_mul_batch(pk, A, B, false, pvac_hip::device_random);
    double best[2] = {1e30, 1e30}, plan[2] = {0, 0};
    for (int round = 0; round < 3; ++round)
        for (int k = 0; k < 2; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            const auto C = k ? pvac_hip::ct_mul_batch(pk, A, B, false, pvac_hip::device_random)
                             : pvac_hip::ct_mul_batch(pk, A, B, false, pvac_hip::os_random_u64);
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            MUST(C.size() == n, "ct_mul_batch size");
            if (sec < best[k]) {
                best[k] = sec;
                plan[k] = pvac_hip::engine_for(pk).last_phases().plan;   // the phase that holds the nonces
            }
        }
    std::printf("{\"pairs\": %zu, \"os_random_u64\": {\"seconds\": %.6f, \"ct_mul_per_s\": %.1f, \"plan_phase_s\": %.6f}, "
                "\"device_random\": {\"seconds\": %.6f, \"ct_mul_per_s\": %.1f, \"plan_phase_s\": %.6f}}\n",
                n, best[0], n / best[0], plan[0], best[1], n / best[1], plan[1]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--time") return time_sources(std::strtoull(argv[2], nullptr, 10));
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s <golden_dir> <canon_tag> <H_digest_hex> <v0>\n", argv[0]);
        return 2;
    }
    const std::string gold = argv[1], ref = gold + "/ref";
    mirror::PubKey pk;
    pk.canon_tag = std::strtoull(argv[2], nullptr, 10);
    const std::string hdig = argv[3];
    for (int i = 0; i < 32; ++i) pk.H_digest[i] = (uint8_t)std::strtoul(hdig.substr(2 * i, 2).c_str(), nullptr, 16);
    const auto pg = read_u64(ref + "/powg_B.u64");
    for (size_t i = 0; i + 1 < pg.size(); i += 2) pk.powg_B.push_back(mirror::Fp{pg[i], pg[i + 1]});
    mirror::SecKey sk;
    const auto kk = read_u64(ref + "/sk_prf_k.u64");
    MUST(kk.size() == 4, "sk_prf_k.u64");
    for (int i = 0; i < 4; ++i) sk.prf_k[i] = kk[i];
    sk.lpn_s_bits = read_u64(ref + "/sk_lpn_s.u64");

    // the RandomSource forms are untouched: the reference's streams replayed give the reference's files
    {
        const Cipher x = read_ct(ref + "/pair0_x.ct")[0], y = read_ct(ref + "/pair0_y.ct")[0];
        replay rs{read_u64(ref + "/pair0_mul_stream.u64")};
        const std::vector<Cipher> A{x}, B{y};
        const Cipher m = pvac_hip::ct_mul_batch(pk, A, B, true, std::ref(rs))[0];
        MUST(rs.k == rs.s.size(), "ct_mul_batch consumed %zu of %zu random words", rs.k, rs.s.size());
        MUST(write_ct({ct_view(m)}) == slurp(ref + "/pair0_mul.ct"), "ct_mul_batch(RandomSource) pair 0 .ct bytes");
        replay_pad re{read_u64(ref + "/enc0_stream.u64")};
        const uint64_t v0 = std::strtoull(argv[4], nullptr, 10);
        const Cipher c = pvac_hip::enc_value_batch<Cipher>(pk, sk, {v0}, true, std::ref(re))[0];
        MUST(re.k >= re.s.size(), "enc_value_batch consumed %zu of %zu words", re.k, re.s.size());
        MUST(write_ct({c}) == slurp(ref + "/enc0.ct"), "enc_value_batch(RandomSource) .ct bytes");
    }

    // enc_value_batch(device_random) round-trips, and two calls never give the same cipher
    constexpr size_t n = 32;
    std::vector<uint64_t> va(n), vb(n);
    for (size_t i = 0; i < n; ++i) {
        va[i] = 0x9E3779B9u * (i + 1) % 0x7FFFFFFFu;
        vb[i] = 0x85EBCA6Bu * (i + 3) % 0x7FFFFFFFu;
    }
    va[0] = 0;   // enc_zero
    const std::vector<Cipher> A = pvac_hip::enc_value_batch<Cipher>(pk, sk, va, false, pvac_hip::device_random);
    const std::vector<Cipher> B = pvac_hip::enc_value_batch<Cipher>(pk, sk, vb, false, pvac_hip::device_random);
    const std::vector<Cipher> A2 = pvac_hip::enc_value_batch<Cipher>(pk, sk, va, false, pvac_hip::device_random);
    MUST(A.size() == n && B.size() == n && A2.size() == n, "enc_value_batch sizes");
    const auto da = pvac_hip::dec_value_batch(pk, sk, A), db = pvac_hip::dec_value_batch(pk, sk, B);
    for (size_t i = 0; i < n; ++i) {
        MUST(da[i].lo == va[i] && da[i].hi == 0 && db[i].lo == vb[i] && db[i].hi == 0, "dec(enc_value_batch(device_random)) %zu", i);
        MUST(!same_edges(A[i], A2[i], false), "two encryptions of value %zu are one cipher", i);
    }
    {   // with sigma: every edge carries m_bits of it
        const std::vector<Cipher> S = pvac_hip::enc_value_batch<Cipher>(pk, sk, {7, 8}, true, pvac_hip::device_random);
        const auto ds = pvac_hip::dec_value_batch(pk, sk, S);
        MUST(ds[0].lo == 7 && ds[1].lo == 8, "dec(enc_value_batch(device_random, sigma))");
        for (const auto& e : S[0].E) MUST(e.s.nbits == (size_t)pk.prm.m_bits, "sigma bits");
    }

    // ct_mul_batch(device_random), with sigma: every product decrypts right, and the salts move on between
    // calls (a commitment covers weights, BASE seeds and sigmas; a PROD layer's nonce is not part of it)
    const std::vector<Cipher> P = pvac_hip::ct_mul_batch(pk, A, B, true, pvac_hip::device_random);
    const std::vector<Cipher> P2 = pvac_hip::ct_mul_batch(pk, A, B, true, pvac_hip::device_random);
    const auto dp = pvac_hip::dec_value_batch(pk, sk, P), dp2 = pvac_hip::dec_value_batch(pk, sk, P2);
    const auto c1 = pvac_hip::commit_ct_batch(pk, P), c2 = pvac_hip::commit_ct_batch(pk, P2);
    for (size_t i = 0; i < n; ++i) {
        MUST(dp[i].lo == va[i] * vb[i] && dp[i].hi == 0, "dec(ct_mul_batch(device_random)) %zu", i);
        MUST(dp2[i].lo == va[i] * vb[i] && dp2[i].hi == 0, "dec(ct_mul_batch(device_random)) second call %zu", i);
        MUST(c1[i] != c2[i], "commit_ct of pair %zu is the same after two calls", i);
        for (const auto& e : P[i].E) MUST(e.s.nbits == (size_t)pk.prm.m_bits, "sigma bits of a product");
        bool nonce_moved = false;   // the nonces too
        for (size_t l = 0; l < P[i].L.size() && l < P2[i].L.size(); ++l)
            nonce_moved |= P[i].L[l].rule == mirror::RRule::PROD && (P[i].L[l].seed.nonce.lo != P2[i].L[l].seed.nonce.lo ||
                                                                     P[i].L[l].seed.nonce.hi != P2[i].L[l].seed.nonce.hi);
        MUST(nonce_moved, "pair %zu drew the same nonces twice", i);
    }
    {   // weights only
        const std::vector<Cipher> W = pvac_hip::ct_mul_batch(pk, A, B, false, pvac_hip::device_random);
        const auto dw = pvac_hip::dec_value_batch(pk, sk, W);
        for (size_t i = 0; i < n; ++i) MUST(dw[i].lo == va[i] * vb[i] && dw[i].hi == 0, "dec(ct_mul_batch(device_random, weights)) %zu", i);
    }
    // a chain on the workers' generators: c_1 = x * x
    {
        const std::vector<Cipher> xs(B.begin(), B.begin() + 4);
        const std::vector<Cipher> C = pvac_hip::ct_mul_chain(pk, xs, 1, false, pvac_hip::device_random);
        const auto dc = pvac_hip::dec_value_batch(pk, sk, C);
        for (size_t i = 0; i < 4; ++i) MUST(dc[i].lo == vb[i] * vb[i] && dc[i].hi == 0, "dec(ct_mul_chain(device_random)) %zu", i);
    }
    std::printf("test_drbg: %d checks passed\n", g_checks);
    return 0;
}
