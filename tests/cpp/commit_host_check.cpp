// commit_host_check.cpp — csrc/commit_msg.hpp's feeder (the code each lane of k_commit_ct runs)
// instantiated on the host, without a GPU:
//   commit_host_check <canon_tag> <H_digest_hex> [<file.ct>:<0|1 with sigma>:<digest_hex>] ...
// every cipher of every file must hash to its reference-minted digest; then a sweep over message
// lengths, field values and sigma widths against a byte-wise SHA-256 written here. Built as a
// stand-alone host program with ASan + UBSan (tests/test_commit_host.py).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "commit_msg.hpp"

using namespace pvhip;

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

// ---- the reference of the sweep: the message as a byte vector, hashed byte-wise (FIPS 180-4)
static void ref_sha256(const std::vector<uint8_t>& msg, uint8_t out[32]) {
    std::vector<uint8_t> m = msg;
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    const uint64_t bits = (uint64_t)msg.size() * 8;
    for (int i = 7; i >= 0; --i) m.push_back((uint8_t)(bits >> (8 * i)));
    sha_state st;
    sha_init(st);
    for (size_t o = 0; o < m.size(); o += 64) {
        uint32_t blk[16];
        for (int i = 0; i < 16; ++i)
            blk[i] = (uint32_t)m[o + 4 * i] << 24 | (uint32_t)m[o + 4 * i + 1] << 16 | (uint32_t)m[o + 4 * i + 2] << 8 | m[o + 4 * i + 3];
        sha_compress(st, blk);
    }
    for (int i = 0; i < 8; ++i)
        for (int b = 0; b < 4; ++b) out[4 * i + b] = (uint8_t)(st.h[i] >> (24 - 8 * b));
}

static void le64(std::vector<uint8_t>& m, uint64_t x) {
    for (int i = 0; i < 8; ++i) m.push_back((uint8_t)(x >> (8 * i)));
}

static std::vector<uint8_t> ref_message(const uint8_t Hd[32], uint64_t canon, const pvac_ct_batch& X, uint64_t i, uint32_t m_bits) {
    std::vector<uint8_t> m;
    const char* lab = "pvac.dom.commit";
    m.insert(m.end(), lab, lab + 15);
    m.insert(m.end(), Hd, Hd + 32);
    le64(m, canon);
    for (uint64_t l = 0; l < X.l_cnt[i]; ++l) {
        const pvac_layer& L = X.layers[X.l_off[i] + l];
        m.push_back((uint8_t)L.rule);
        if (L.rule == 0) { le64(m, L.ztag); le64(m, L.nonce_lo); le64(m, L.nonce_hi); }
        else { le64(m, L.pa); le64(m, L.pb); }
    }
    for (uint64_t e = 0; e < X.e_cnt[i]; ++e) {
        const uint64_t s = X.e_off[i] + e, mt = X.meta[s];
        le64(m, (uint32_t)mt);
        le64(m, (uint16_t)(mt >> 32));
        m.push_back((uint8_t)(mt >> 48));
        le64(m, X.w_lo[s]);
        le64(m, X.w_hi[s] & 0x7FFFFFFFFFFFFFFFull);
        if (X.sigma)
            for (uint32_t b = 0; b < (m_bits + 7) / 8; ++b)
                m.push_back((uint8_t)(X.sigma[s * X.sigma_words + (b >> 3)] >> (8 * (b & 7))));
    }
    return m;
}

static void feeder_digest(const uint8_t Hd[32], uint64_t canon, const pvac_ct_batch& X, uint64_t i, uint32_t m_bits, uint8_t out[32]) {
    uint32_t head[kCommitHeadWords];
    commit_head_words(Hd, canon, head);
    commit_host_ring ring;
    const commit_cipher c = commit_cipher_of(X, i, X.sigma ? (m_bits + 7) / 8 : 0);
    commit_one(ring, head, c, out);
}

static std::string hex(const uint8_t d[32]) {
    char s[65];
    for (int i = 0; i < 32; ++i) std::snprintf(s + 2 * i, 3, "%02x", d[i]);
    return s;
}

// ---- host batches
struct host_batch {
    std::vector<uint64_t> l_off, l_cnt, e_off, e_cnt, meta, w_lo, w_hi, sigma;
    std::vector<pvac_layer> layers;
    uint32_t sigma_words = 0;
    pvac_ct_batch view(bool with_sigma) {
        pvac_ct_batch v{};
        v.n = l_off.size();
        v.l_off = l_off.data(); v.l_cnt = l_cnt.data(); v.layers = layers.data();
        v.e_off = e_off.data(); v.e_cnt = e_cnt.data();
        v.meta = meta.data(); v.w_lo = w_lo.data(); v.w_hi = w_hi.data();
        v.sigma = with_sigma ? sigma.data() : nullptr;
        v.sigma_words = sigma_words;
        return v;
    }
};

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static uint64_t rnd() {
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

// a cipher of nL layers (every `prod_every`-th a PROD layer, 0 = none) and nE edges, `gap` unused
// slots in front of its rows (capacity-padded CSR)
static void add_cipher(host_batch& b, uint32_t nL, uint32_t nE, uint32_t prod_every, uint32_t gap) {
    for (uint32_t g = 0; g < gap; ++g) {
        pvac_layer junk{7, 7, 7, 7, rnd(), rnd(), rnd()};
        b.layers.push_back(junk);
        b.meta.push_back(rnd()); b.w_lo.push_back(rnd()); b.w_hi.push_back(rnd());
        for (uint32_t w = 0; w < b.sigma_words; ++w) b.sigma.push_back(rnd());
    }
    b.l_off.push_back(b.layers.size()); b.l_cnt.push_back(nL);
    b.e_off.push_back(b.meta.size()); b.e_cnt.push_back(nE);
    for (uint32_t l = 0; l < nL; ++l) {
        pvac_layer L{};
        const bool prod = prod_every && l % prod_every == prod_every - 1;
        L.rule = prod ? 1 : 0;
        L.pa = (uint32_t)rnd(); L.pb = (uint32_t)rnd(); L.pad = (uint32_t)rnd();
        L.ztag = rnd(); L.nonce_lo = rnd(); L.nonce_hi = rnd();
        b.layers.push_back(L);
    }
    for (uint32_t e = 0; e < nE; ++e) {
        // layer ids above 2^16, idx up to 65,535, ch 0 / 1, bits 56-63 of meta set (not hashed)
        const uint64_t lid = rnd() & 0xFFFFFFFFull, idx = e % 3 ? rnd() & 0xFFFF : 65535, ch = rnd() & 1;
        b.meta.push_back(lid | idx << 32 | ch << 48 | (rnd() & 0xFFull) << 56);
        b.w_lo.push_back(rnd());
        b.w_hi.push_back(rnd() | (e & 1 ? 1ull << 63 : 0));   // bit 63 set: the mask applies
        for (uint32_t w = 0; w < b.sigma_words; ++w) b.sigma.push_back(rnd());
    }
}

static void check_batch(host_batch& b, bool with_sigma, uint32_t m_bits, const char* what) {
    uint8_t Hd[32];
    for (int i = 0; i < 32; ++i) Hd[i] = (uint8_t)rnd();
    const uint64_t canon = rnd();
    const pvac_ct_batch X = b.view(with_sigma);
    for (uint64_t i = 0; i < X.n; ++i) {
        uint8_t want[32], got[32];
        const std::vector<uint8_t> msg = ref_message(Hd, canon, X, i, m_bits);
        ref_sha256(msg, want);
        feeder_digest(Hd, canon, X, i, m_bits, got);
        MUST(std::memcmp(want, got, 32) == 0, "%s: cipher %" PRIu64 " (%zu message bytes): %s != %s", what, i, msg.size(),
             hex(got).c_str(), hex(want).c_str());
    }
}

static std::vector<uint8_t> slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    MUST(f.good(), "open %s", p.c_str());
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <canon_tag> <H_digest_hex> [<file.ct>:<0|1>:<digest_hex>] ...\n", argv[0]);
        return 2;
    }
    const uint64_t canon = std::strtoull(argv[1], nullptr, 10);
    uint8_t Hd[32];
    MUST(std::strlen(argv[2]) == 64, "H_digest");
    for (int i = 0; i < 32; ++i) Hd[i] = (uint8_t)std::strtoul(std::string(argv[2] + 2 * i, 2).c_str(), nullptr, 16);

    // ---- reference-minted digests of the fixture files
    int fixtures = 0;
    for (int a = 3; a < argc; ++a) {
        const std::string s = argv[a];
        const size_t c2 = s.rfind(':'), c1 = s.rfind(':', c2 - 1);
        MUST(c1 != std::string::npos && c2 != std::string::npos && c2 > c1, "argument %s", s.c_str());
        const std::string path = s.substr(0, c1), want = s.substr(c2 + 1);
        const bool with_sigma = s[c1 + 1] == '1';
        const std::vector<uint8_t> buf = slurp(path);
        pvac_ct_file_info info{};
        MUST(pvac_ct_scan(buf.data(), buf.size(), &info) == PVAC_OK, "scan %s", path.c_str());
        MUST(info.n_ciphers == 1, "%s holds %" PRIu64 " ciphers", path.c_str(), info.n_ciphers);
        MUST(!with_sigma || info.sigma_bits == 8192, "%s carries sigma of %u bits", path.c_str(), info.sigma_bits);
        host_batch b;
        b.l_off.resize(1); b.l_cnt.resize(1); b.e_off.resize(1); b.e_cnt.resize(1);
        b.layers.resize(info.total_layers);
        b.meta.resize(info.total_edges); b.w_lo.resize(info.total_edges); b.w_hi.resize(info.total_edges);
        b.sigma_words = info.sigma_words;
        b.sigma.resize(info.total_edges * info.sigma_words);
        pvac_ct_batch X = b.view(info.sigma_words != 0);
        MUST(pvac_ct_parse(buf.data(), buf.size(), &X, 1) == PVAC_OK, "parse %s", path.c_str());
        if (!with_sigma) X.sigma = nullptr;
        uint8_t got[32];
        feeder_digest(Hd, canon, X, 0, 8192, got);
        MUST(hex(got) == want, "%s (%s): %s, the reference minted %s", path.c_str(), with_sigma ? "with sigma" : "weights only",
             hex(got).c_str(), want.c_str());
        ++fixtures;
    }

    // ---- length sweep, weights only: one BASE layer and e = 0..63 edges give 80 + 33 e bytes, every
    // residue modulo 64; the empty cipher's 55 bytes are padded to exactly one block; 56 bytes modulo
    // 64 spill the length into another block (e = 40: 1400 = 21 * 64 + 56); PROD layers mixed in;
    // rows behind gaps
    {
        host_batch b;
        add_cipher(b, 0, 0, 0, 0);                                        // 55 bytes
        for (uint32_t e = 0; e < 64; ++e) add_cipher(b, 1, e, 0, e % 5);  // 80 + 33 e
        for (uint32_t e = 0; e < 64; ++e) add_cipher(b, 2 + e % 7, e, 2 + e % 3, (e + 1) % 4);
        add_cipher(b, 5, 0, 2, 3);                                        // layers only
        check_batch(b, false, 8192, "length sweep");
        bool r55 = false, r56 = false;
        std::vector<bool> residues(64, false);
        uint8_t Hz[32] = {0};
        for (uint64_t i = 0; i < b.l_off.size(); ++i) {
            const size_t len = ref_message(Hz, 0, b.view(false), i, 8192).size();
            residues[len % 64] = true;
            r55 |= len == 55;
            r56 |= len % 64 == 56;
        }
        MUST(r55 && r56, "the sweep holds the 55-byte and the 56-modulo-64 messages");
        for (int k = 0; k < 64; ++k) MUST(residues[k], "residue %d not covered", k);
    }
    // ---- sigma widths: full rows at two strides, a partial word, a partial byte
    {
        const struct { uint32_t m_bits, stride; } widths[] = {{8192, 128}, {8192, 130}, {8200, 129}, {100, 2}, {8, 1}, {64, 1},
                                                                 {520, 9}, {513, 9}, {1016, 16}};
        for (const auto& w : widths) {
            host_batch b;
            b.sigma_words = w.stride;
            for (uint32_t e = 0; e < 6; ++e) add_cipher(b, 1 + e % 3, e, e % 2 ? 2 : 0, e % 3);
            char what[64];
            std::snprintf(what, sizeof what, "sigma m_bits %u stride %u", w.m_bits, w.stride);
            check_batch(b, true, w.m_bits, what);
            check_batch(b, false, w.m_bits, what);
        }
    }
    std::printf("commit_host_check: ok (%d fixture digests, %d checks)\n", fixtures, g_checks);
    return 0;
}
