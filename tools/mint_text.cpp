// mint_text.cpp — TEST INFRASTRUCTURE ONLY: mints tests/golden/text/ with the unmodified reference's
// enc_text (utils/text.hpp:39-61) and enc_fp_depth (ops/encrypt.hpp:162-258). The engine never links,
// loads or calls it.
//
//   g++ -std=c++17 -O2 -march=native -w -I<reference>/include -pthread \
//       -o oracle/_ref/mint_text tools/mint_text.cpp
//   oracle/_ref/mint_text tests/golden/ref tests/golden/text
//   oracle/_ref/mint_text tests/golden/ref --time [messages]     (enc_text of 150-byte messages, one core)
//   oracle/_ref/mint_text tests/golden/ref --dec <file.ct>       (the reference's dec_text of a file, as hex)
//
// Determinism as in tools/mint_recrypt.cpp: getrandom(2) is interposed with a seeded splitmix64
// stream whose words are logged (word j after a reseed is splitmix64(seed + (j + 1) * golden)). The
// key is the fixture key (reseed 0x5EED0C00 before keygen); nothing is written unless canon_tag and
// H_digest equal <golden ref>/manifest.json.
//
// Every message is encrypted twice from the same seed: once by enc_text, once piecewise (enc_value of
// the length, then enc_fp_depth per block with hints 2, 3, ...), noting the log position at every
// cipher boundary; the two outputs must be equal, which makes the positions each cipher's exact draw
// segment. Output per case <name>: the ciphers as <name>.ct with sigmas (messages up to 31 bytes and
// the fpraw set) or weights-only in parts <name>_p<k>.ct of at most 48 ciphers (the long messages),
// the draw log <name>.u64 when it has at most 8192 words (a longer one is regenerated from the seed),
// and in manifest.json the message, the seed, the noise Params and per cipher: kind, hint, plaintext
// words, draw segment, edges and commit_ct (always taken with sigmas).
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

static std::vector<Cipher> read_ct(const std::string& path, int m_bits) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); std::exit(2); }
    auto g32 = [&] { uint32_t x = 0; f.read((char*)&x, 4); return x; };
    auto g64 = [&] { uint64_t x = 0; f.read((char*)&x, 8); return x; };
    if (g32() != 0x66699666u || g32() != 1u) { std::fprintf(stderr, "bad file %s\n", path.c_str()); std::exit(2); }
    std::vector<Cipher> out(g64());
    for (Cipher& C : out) {
        const uint32_t nL = g32(), nE = g32();
        for (uint32_t i = 0; i < nL; ++i) {
            Layer L{};
            L.rule = (RRule)f.get();
            if (L.rule == RRule::BASE) {
                L.seed.ztag = g64();
                L.seed.nonce.lo = g64();
                L.seed.nonce.hi = g64();
            } else {
                L.pa = g32();
                L.pb = g32();
            }
            C.L.push_back(L);
        }
        for (uint32_t i = 0; i < nE; ++i) {
            Edge e{};
            e.layer_id = g32();
            f.read((char*)&e.idx, 2);
            e.ch = (uint8_t)f.get();
            f.get();
            e.w.lo = g64();
            e.w.hi = g64();
            const uint32_t nbits = g32();
            e.s = BitVec::make(m_bits);
            for (size_t w = 0; w < (nbits + 63) / 64; ++w) e.s.w[w] = g64();
            C.E.push_back(e);
        }
    }
    return out;
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

static const size_t kPart = 48, kLogMax = 8192;

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
    js << "    {\"name\": \"" << k.name << "\", \"kind\": \"" << (k.text ? "text" : "fpraw") << "\", \"msg_hex\": \""
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
    if (argc < 3) { std::fprintf(stderr, "usage: %s <golden ref dir> <out dir> | <golden ref dir> --time [messages]\n", argv[0]); return 2; }
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
    if (dir == "--dec") {
        if (argc < 4) { std::fprintf(stderr, "--dec <file.ct>\n"); return 2; }
        const std::string msg = dec_text(pk, sk, read_ct(argv[3], prm.m_bits));
        std::printf("dec_text %s\n", hex((const uint8_t*)msg.data(), msg.size()).c_str());
        return 0;
    }
    if (dir == "--time") {
        const int n = argc > 3 ? std::atoi(argv[3]) : 32;
        std::string msg(150, 'x');
        for (size_t i = 0; i < msg.size(); ++i) msg[i] = (char)(32 + (i * 7) % 90);
        g_logging = false;
        g_state = 0x5EED7100ULL;
        size_t ciphers = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < n; ++i) ciphers += enc_text(pk, sk, msg).size();
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("{\"messages\": %d, \"bytes_each\": 150, \"ciphers\": %zu, \"seconds\": %.6f, \"ciphers_per_s\": %.2f, "
                    "\"bytes_per_s\": %.1f}\n", n, ciphers, s, ciphers / s, n * 150.0 / s);
        return 0;
    }

    auto text_case = [&](const std::string& name, const std::string& msg, bool sigma, uint64_t seed, double nb, double t2,
                         double slope) {
        PubKey q = pk;
        q.prm.noise_entropy_bits = nb;
        q.prm.tuple2_fraction = t2;
        q.prm.depth_slope_bits = slope;
        Case k{name, msg, true, sigma, seed, nb, t2, slope, {}, {}, 0};
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

    std::string m15("fifteen bytes!!"), m16(16, '\0'), m30, m31, m240, m1845;
    m16[0] = (char)0xFF; m16[7] = (char)0xFF; m16[8] = (char)0x01; m16[14] = (char)0xFF; m16[15] = (char)0x00;   // trailing zero
    for (int i = 0; i < 30; ++i) m30 += (char)(i % 3 == 0 ? 0x00 : (i % 3 == 1 ? 0xFF : 0x41 + i));
    m30[28] = 0; m30[29] = 0;   // trailing zero bytes inside the last block
    for (int i = 0; i < 31; ++i) m31 += (char)(0xF0 + (i & 15));
    for (int i = 0; i < 240; ++i) m240 += (char)((i * 37 + 11) & 0xFF);
    for (int i = 0; i < 1845; ++i) m1845 += (char)((i * 101 + (i >> 8) * 17 + 3) & 0xFF);
    const std::string utf8 = "Gr\xC3\xBC\xC3\x9F" "e, \xE4\xB8\x96\xE7\x95\x8C \xF0\x9F\x94\x90";

    std::vector<Case> cases;
    const double NB = 120.0, T2 = 0.55, SL = 16.0;
    cases.push_back(text_case("empty", "", true, 0x5EED7000ULL, NB, T2, SL));
    cases.push_back(text_case("one", std::string(1, '\xA5'), true, 0x5EED7001ULL, NB, T2, SL));
    cases.push_back(text_case("b15", m15, true, 0x5EED7002ULL, NB, T2, SL));
    cases.push_back(text_case("b16", m16, true, 0x5EED7003ULL, NB, T2, SL));
    cases.push_back(text_case("b30", m30, true, 0x5EED7004ULL, NB, T2, SL));
    cases.push_back(text_case("b31", m31, true, 0x5EED7005ULL, NB, T2, SL));
    cases.push_back(text_case("utf8", utf8, true, 0x5EED7006ULL, NB, T2, SL));
    cases.push_back(text_case("b240", m240, false, 0x5EED7007ULL, NB, T2, SL));
    cases.push_back(text_case("b1845", m1845, false, 0x5EED7008ULL, NB, T2, SL));
    // no noise group at any hint; and hint 0 without groups next to blocks whose single group is bumped to two
    cases.push_back(text_case("nonoise", "no noise groups at all", true, 0x5EED7009ULL, 0.0, 0.55, 0.0));
    cases.push_back(text_case("bump", "z2 + z3 == 1 is bumped", true, 0x5EED700AULL, 0.0, 0.55, 16.0));
    {   // direct enc_fp_depth(v, 3) on plaintext words as given, canonical or not
        const uint64_t A = ~0ull, M = 0x7FFFFFFFFFFFFFFFULL;
        const Fp vs[6] = {{0, 0}, {1, 0}, {A - 1, M}, {A, M}, {0, 1ull << 63}, {A, A}};
        Case k{"fpraw", "", false, true, 0x5EED700BULL, NB, T2, SL, {}, {}, 0};
        g_state = k.seed;
        g_log.clear();
        for (const Fp& v : vs) {
            const size_t at = g_log.size();
            k.cts.push_back(enc_fp_depth(pk, sk, v, 3));
            k.items.push_back({0, 3, v, at, g_log.size() - at});
        }
        k.draws = g_log.size();
        cases.push_back(k);
    }

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
