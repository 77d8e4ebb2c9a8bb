// mint_text_wide.cpp — TEST INFRASTRUCTURE ONLY: mints tests/golden/text_wide/ with the unmodified
// reference's enc_text (utils/text.hpp:39-61), enc_fp_depth, enc_value_depth and enc_zero_depth
// (ops/encrypt.hpp:162-258, 281-298) at noise plans above 256 pre-merge edges per half, which
// tools/mint_text.cpp does not reach. The engine never links, loads or calls it.
//
//   g++ -std=c++17 -O2 -march=native -w -I<reference>/include -pthread \
//       -o oracle/_ref/mint_text_wide tools/mint_text_wide.cpp
//   oracle/_ref/mint_text_wide tests/golden/ref tests/golden/text_wide
//   oracle/_ref/mint_text_wide tests/golden/ref --time [bytes]   (one enc_text of a message, one core; 3000 bytes)
//
// Determinism, the fixture-key check and the manifest are those of tools/mint_text.cpp: getrandom(2) is
// interposed with a seeded splitmix64 stream whose words are logged, every case starts at word 0 of
// its seed, a text is encrypted twice (enc_text, then piecewise, which gives every cipher's draw
// segment) and the two must agree. Every case is stored weights-only in parts <name>_p<k>.ct of at
// most 24 ciphers; commit_ct in the manifest is taken with sigmas. Draw logs of at most 8192 words are
// stored as <name>.u64, longer ones are regenerated from the seed. Cases:
//   fpwide   enc_fp_depth at hints 125, 126 (the first with a new Z3), 200, 400 (782 edges on 674 keys),
//            1000; the plaintexts include a non-canonical word pair
//   valwide  enc_value_depth at hints 125 and 300, enc_zero_depth at 125
//   b1875    a 1,875-byte message, 125 blocks: its last two ciphers (hints 125, 126) are wide
//   steep    a 75-byte message under noise (120, 0.55, 400): hints 5 (257 edges) and 6 (307) are wide
//   t2one, t2zero   enc_fp_depth at hint 125 with tuple2_fraction 1.0 and 0.0: Z2-only and Z3-only plans
#include <pvac/pvac.hpp>
#include <pvac/utils/text.hpp>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace pvac;

static uint64_t g_state = 1;
static std::vector<uint64_t> g_log;
static bool g_logging = true;

extern "C" ssize_t getrandom(void* buf, size_t n, unsigned int) {
    uint8_t* p = (uint8_t*)buf;
    for (size_t off = 0; off < n; off += 8) {
        uint64_t z = (g_state += 0x9e3779b97f4a7c15ULL);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        z ^= z >> 31;
        if (g_logging) g_log.push_back(z);
        std::memcpy(p + off, &z, n - off < 8 ? n - off : 8);
    }
    return (ssize_t)n;
}

static void put32(std::ostream& o, uint32_t x) { o.write((const char*)&x, 4); }
static void put64(std::ostream& o, uint64_t x) { o.write((const char*)&x, 8); }

// the reference's .ct layout (tests/add.cpp:22-155)
static void write_ct(std::ostream& o, const Cipher* cts, size_t n, bool with_sigma) {
    put32(o, 0x66699666u);
    put32(o, 1u);
    put64(o, (uint64_t)n);
    for (size_t c = 0; c < n; ++c) {
        const Cipher& C = cts[c];
        put32(o, (uint32_t)C.L.size());
        put32(o, (uint32_t)C.E.size());
        for (const Layer& L : C.L) {
            o.put((char)(uint8_t)L.rule);
            if (L.rule == RRule::BASE) {
                put64(o, L.seed.ztag);
                put64(o, L.seed.nonce.lo);
                put64(o, L.seed.nonce.hi);
            } else {
                put32(o, L.pa);
                put32(o, L.pb);
            }
        }
        for (const Edge& e : C.E) {
            put32(o, e.layer_id);
            o.write((const char*)&e.idx, 2);
            o.put((char)e.ch);
            o.put(0);
            put64(o, e.w.lo);
            put64(o, e.w.hi);
            put32(o, with_sigma ? (uint32_t)e.s.nbits : 0u);
            if (with_sigma)
                for (size_t i = 0; i < (e.s.nbits + 63) / 64; ++i) put64(o, e.s.w[i]);
        }
    }
}

static std::string bytes_of(const std::vector<Cipher>& cts) {
    std::ostringstream o;
    write_ct(o, cts.data(), cts.size(), true);
    return o.str();
}

static std::string hex(const uint8_t* d, size_t n) {
    static const char* H = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) { s += H[d[i] >> 4]; s += H[d[i] & 15]; }
    return s;
}

struct Item {
    int kind, hint;   // 0 = enc_fp_depth, 1 = enc_value
    Fp v;
    size_t off, cnt;
};

struct Case {
    std::string name, msg;
    bool text, sigma;
    uint64_t seed;
    double nb, t2, slope;
    std::vector<Cipher> cts;
    std::vector<Item> items;
    size_t draws;
};

static const size_t kPart = 24, kLogMax = 8192;

static bool emit(const std::string& dir, const PubKey& pk, Case& k, std::ostringstream& js, bool last) {
    if (k.sigma) {
        std::ofstream o(dir + "/" + k.name + ".ct", std::ios::binary);
        write_ct(o, k.cts.data(), k.cts.size(), true);
    } else {
        for (size_t p = 0; p * kPart < k.cts.size(); ++p) {
            std::ofstream o(dir + "/" + k.name + "_p" + std::to_string(p) + ".ct", std::ios::binary);
            write_ct(o, k.cts.data() + p * kPart, std::min(kPart, k.cts.size() - p * kPart), false);
        }
    }
    const bool log_file = k.draws <= kLogMax;
    if (log_file) {
        std::ofstream o(dir + "/" + k.name + ".u64", std::ios::binary);
        o.write((const char*)g_log.data(), (std::streamsize)(k.draws * 8));
    }
    js << "    {\"name\": \"" << k.name << "\", \"kind\": \"" << (k.text ? "text" : "items") << "\", \"msg_hex\": \""
       << hex((const uint8_t*)k.msg.data(), k.msg.size()) << "\", \"sigma\": " << (k.sigma ? "true" : "false")
       << ", \"seed\": " << k.seed << ", \"draws\": " << k.draws << ", \"log_file\": " << (log_file ? "true" : "false")
       << ", \"parts\": " << (k.sigma ? 0 : (k.cts.size() + kPart - 1) / kPart) << ", \"part_ciphers\": " << kPart
       << ",\n     \"noise_entropy_bits\": " << k.nb << ", \"tuple2_fraction\": " << k.t2 << ", \"depth_slope_bits\": " << k.slope
       << ", \"ciphers\": [\n";
    for (size_t i = 0; i < k.items.size(); ++i) {
        const Item& it = k.items[i];
        const auto cm = commit_ct(pk, k.cts[i]);
        js << "      {\"kind\": " << it.kind << ", \"hint\": " << it.hint << ", \"v_lo\": " << it.v.lo << ", \"v_hi\": " << it.v.hi
           << ", \"off\": " << it.off << ", \"cnt\": " << it.cnt << ", \"layers\": " << k.cts[i].L.size() << ", \"edges\": "
           << k.cts[i].E.size() << ", \"commit\": \"" << hex(cm.data(), 32) << "\"}" << (i + 1 < k.items.size() ? "," : "")
           << "\n";
    }
    js << "    ]}" << (last ? "" : ",") << "\n";
    std::printf("%-10s %4zu bytes, %3zu ciphers, %6zu draws%s\n", k.name.c_str(), k.msg.size(), k.cts.size(), k.draws,
                k.sigma ? ", sigma" : "");
    return true;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <golden ref dir> <out dir> | <golden ref dir> --time [bytes]\n", argv[0]); return 2; }
    const std::string ref = argv[1], dir = argv[2];
    g_state = 0x5EED0C00ULL;
    Params prm;
    PubKey pk;
    SecKey sk;
    keygen(prm, pk, sk);
    {   // the fixture key, or nothing is written
        std::ifstream f(ref + "/manifest.json");
        std::stringstream ss;
        ss << f.rdbuf();
        const std::string man = ss.str();
        if (man.find("\"canon_tag\": " + std::to_string(pk.canon_tag) + ",") == std::string::npos ||
            man.find("\"H_digest\": \"" + hex(pk.H_digest.data(), 32) + "\"") == std::string::npos) {
            std::fprintf(stderr, "this key is not the fixture key of %s/manifest.json\n", ref.c_str());
            return 1;
        }
    }
    // the first encryption of a process also picks the PRF's Toeplitz implementation by timing it on
    // random inputs: spend those draws here, so that every case below starts at word 0 of its seed
    g_state = 0x5EED70FFULL;
    (void)enc_value(pk, sk, 1);
    auto message = [](size_t n, int a, int b) {
        std::string m;
        for (size_t i = 0; i < n; ++i) m += (char)((i * a + (i >> 8) * b + 3) & 0xFF);
        return m;
    };
    if (dir == "--time") {
        const size_t bytes = argc > 3 ? (size_t)std::atol(argv[3]) : 3000;
        const std::string msg = message(bytes, 101, 17);
        g_logging = false;
        g_state = 0x5EED7100ULL;
        const auto t0 = std::chrono::steady_clock::now();
        const size_t ciphers = enc_text(pk, sk, msg).size();
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("{\"bytes\": %zu, \"ciphers\": %zu, \"seconds\": %.6f, \"bytes_per_s\": %.1f}\n", bytes, ciphers, s, bytes / s);
        return 0;
    }

    const double NB = 120.0, T2 = 0.55, SL = 16.0;
    auto with_noise = [&](double nb, double t2, double slope) {
        PubKey q = pk;
        q.prm.noise_entropy_bits = nb;
        q.prm.tuple2_fraction = t2;
        q.prm.depth_slope_bits = slope;
        return q;
    };
    auto text_case = [&](const std::string& name, const std::string& msg, uint64_t seed, double nb, double t2, double slope) {
        const PubKey q = with_noise(nb, t2, slope);
        Case k{name, msg, true, false, seed, nb, t2, slope, {}, {}, 0};
        g_state = seed;
        g_log.clear();
        const std::vector<Cipher> whole = enc_text(q, sk, msg);
        g_state = seed;
        g_log.clear();
        k.cts.push_back(enc_value(q, sk, (uint64_t)msg.size()));
        k.items.push_back({1, 0, fp_from_u64((uint64_t)msg.size()), 0, g_log.size()});
        int hint = 2;
        for (size_t pos = 0; pos < msg.size(); pos += 15, ++hint) {
            const size_t at = g_log.size();
            const Fp x = pack_15_bytes_to_fp((const uint8_t*)msg.data() + pos, std::min<size_t>(15, msg.size() - pos));
            k.cts.push_back(enc_fp_depth(q, sk, x, hint));
            k.items.push_back({0, hint, x, at, g_log.size() - at});
        }
        k.draws = g_log.size();
        if (bytes_of(whole) != bytes_of(k.cts)) {
            std::fprintf(stderr, "%s: the piecewise run differs from enc_text\n", name.c_str());
            std::exit(1);
        }
        if (dec_text(q, sk, k.cts) != msg) {
            std::fprintf(stderr, "%s: dec_text does not return the message\n", name.c_str());
            std::exit(1);
        }
        return k;
    };
    // items: (kind, hint, plaintext); kind 0 = enc_fp_depth, 1 = enc_value_depth (v = 0: enc_zero_depth)
    auto items_case = [&](const std::string& name, const std::vector<Item>& want, uint64_t seed, double nb, double t2, double slope) {
        const PubKey q = with_noise(nb, t2, slope);
        Case k{name, "", false, false, seed, nb, t2, slope, {}, {}, 0};
        g_state = seed;
        g_log.clear();
        for (const Item& w : want) {
            const size_t at = g_log.size();
            if (w.kind == 0) k.cts.push_back(enc_fp_depth(q, sk, w.v, w.hint));
            else if (w.v.lo == 0) k.cts.push_back(enc_zero_depth(q, sk, w.hint));
            else k.cts.push_back(enc_value_depth(q, sk, w.v.lo, w.hint));
            k.items.push_back({w.kind, w.hint, w.v, at, g_log.size() - at});
            if (w.kind == 1) {   // a masked value decrypts to itself (FP plaintexts may be non-canonical)
                const Fp d = dec_value(q, sk, k.cts.back());
                if (d.lo != w.v.lo || d.hi != 0) {
                    std::fprintf(stderr, "%s: dec_value does not return the plaintext\n", name.c_str());
                    std::exit(1);
                }
            }
        }
        k.draws = g_log.size();
        return k;
    };

    const uint64_t A = ~0ull, M = 0x7FFFFFFFFFFFFFFFULL;
    std::vector<Case> cases;
    cases.push_back(items_case("fpwide", {{0, 125, {0x0123456789ABCDEFull, 0x0FEDCBA987654321ull}, 0, 0},
                                          {0, 126, {A, M}, 0, 0},   // p itself: a non-canonical zero
                                          {0, 200, {7, 1ull << 63}, 0, 0},   // bit 127 set
                                          {0, 400, {0xDEADBEEFCAFEF00Dull, 0x1234ull}, 0, 0},
                                          {0, 1000, {42, 0}, 0, 0}},
                               0x5EED7200ULL, NB, T2, SL));
    cases.push_back(items_case("valwide", {{1, 125, {0xC0FFEEull, 0}, 0, 0}, {1, 300, {A - 5, 0}, 0, 0}, {1, 125, {0, 0}, 0, 0}},
                               0x5EED7201ULL, NB, T2, SL));
    cases.push_back(text_case("b1875", message(1875, 101, 17), 0x5EED7202ULL, NB, T2, SL));
    cases.push_back(text_case("steep", message(75, 37, 5), 0x5EED7203ULL, 120.0, 0.55, 400.0));
    cases.push_back(items_case("t2one", {{0, 125, {0x1111ull, 0x2222ull}, 0, 0}}, 0x5EED7204ULL, 120.0, 1.0, 16.0));
    cases.push_back(items_case("t2zero", {{0, 125, {0x3333ull, 0x4444ull}, 0, 0}}, 0x5EED7205ULL, 120.0, 0.0, 16.0));

    std::ostringstream js;
    js << "{\n  \"canon_tag\": " << pk.canon_tag << ",\n  \"cases\": [\n";
    for (size_t i = 0; i < cases.size(); ++i) {
        // the log of the case, regenerated: emit writes it from g_log
        g_state = cases[i].seed;
        g_log.clear();
        std::vector<uint8_t> sink(cases[i].draws * 8);
        if (!sink.empty()) getrandom(sink.data(), sink.size(), 0);
        emit(dir, pk, cases[i], js, i + 1 == cases.size());
    }
    js << "  ]\n}\n";
    std::ofstream(dir + "/manifest.json") << js.str();
    return 0;
}
