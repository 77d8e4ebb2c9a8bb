// mint_recrypt.cpp — TEST INFRASTRUCTURE ONLY: mints tests/golden/recrypt/ with the unmodified
// reference's ct_recrypt (ops/recrypt.hpp:26-41). The engine never links, loads or calls it.
//
//   g++ -std=c++17 -O2 -march=native -w -I<reference>/include -pthread \
//       -o oracle/_ref/mint_recrypt tools/mint_recrypt.cpp
//   oracle/_ref/mint_recrypt tests/golden/ref tests/golden/recrypt
//
// Determinism as in oracle/ref_harness.cpp: the reference's entropy all comes from getrandom(2)
// (core/random.hpp:40-110), interposed here with a seeded splitmix64 stream whose words are logged,
// so the draws of every ct_recrypt call go into the manifest. The key is the fixture key (reseed
// 0x5EED0C00 before keygen); nothing is written unless canon_tag and H_digest equal
// <golden ref>/manifest.json, so sk_*.u64, powg_B.u64 and the H fixtures apply to these files too.
//
// Output: ubk_inv.i32 (pk.ubk.inv), pool.ct (make_evalkey(pk, sk, 4, 0).zero_pool), per case
// <name>_in.ct / <name>_out.ct with sigmas, the product case (input <golden ref>/pair0_mul.ct) as
// a weights-only <name>_out.ct, and manifest.json: iterations, draws, commit_ct of every output.
#include <pvac/pvac.hpp>

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

extern "C" ssize_t getrandom(void* buf, size_t n, unsigned int) {
    uint8_t* p = (uint8_t*)buf;
    for (size_t off = 0; off < n; off += 8) {
        uint64_t z = (g_state += 0x9e3779b97f4a7c15ULL);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        z ^= z >> 31;
        g_log.push_back(z);
        std::memcpy(p + off, &z, n - off < 8 ? n - off : 8);
    }
    return (ssize_t)n;
}

static void put32(std::ostream& o, uint32_t x) { o.write((const char*)&x, 4); }
static void put64(std::ostream& o, uint64_t x) { o.write((const char*)&x, 8); }

// the reference's .ct layout (tests/add.cpp:22-155)
static void write_ct(const std::string& path, const std::vector<Cipher>& cts, bool with_sigma) {
    std::ofstream o(path, std::ios::binary);
    put32(o, 0x66699666u);
    put32(o, 1u);
    put64(o, (uint64_t)cts.size());
    for (const Cipher& C : cts) {
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

static Cipher read_ct_one(const std::string& path, int m_bits) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); std::exit(2); }
    auto g32 = [&] { uint32_t x = 0; f.read((char*)&x, 4); return x; };
    auto g64 = [&] { uint64_t x = 0; f.read((char*)&x, 8); return x; };
    if (g32() != 0x66699666u || g32() != 1u || g64() < 1) { std::fprintf(stderr, "bad file %s\n", path.c_str()); std::exit(2); }
    Cipher C;
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
    return C;
}

static std::string hex(const uint8_t* d, size_t n) {
    static const char* H = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) { s += H[d[i] >> 4]; s += H[d[i] & 15]; }
    return s;
}

struct Result {
    Cipher out;
    int iterations;
    std::vector<uint64_t> draws;
};

static Result run(const PubKey& pk, const EvalKey& ek, const Cipher& in, uint64_t seed) {
    g_state = seed;
    g_log.clear();
    Result r;
    r.out = ct_recrypt(pk, ek, in);
    r.draws = g_log;              // one csprng_u64 per iteration that ran, nothing else draws
    r.iterations = (int)r.draws.size();
    return r;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <golden ref dir> <out dir>\n", argv[0]); return 2; }
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
    g_state = 0x5EED0A00ULL;
    const EvalKey ek = make_evalkey(pk, sk, 4, 0);
    write_ct(dir + "/pool.ct", ek.zero_pool, true);
    {
        std::vector<int32_t> inv(pk.ubk.inv.begin(), pk.ubk.inv.end());
        std::ofstream o(dir + "/ubk_inv.i32", std::ios::binary);
        o.write((const char*)inv.data(), (std::streamsize)(inv.size() * 4));
    }
    g_state = 0x5EED0A10ULL;
    const Cipher fresh = enc_value(pk, sk, 123456789);
    auto skewed = [&](size_t k) {   // s &= rotl(s, 1) on the first k edges
        Cipher c = fresh;
        for (size_t i = 0; i < k && i < c.E.size(); ++i)
            for (uint64_t& w : c.E[i].s.w) w &= (w << 1) | (w >> 63);
        return c;
    };
    struct Case { std::string name; Cipher in; bool sigma; };
    std::vector<Case> cases;
    cases.push_back({"fresh", fresh, true});
    // the smallest skews that take exactly one iteration and a middle count, then all-zero sigmas (8)
    bool have_one = false, have_mid = false;
    for (size_t k = 1; k <= fresh.E.size() && !(have_one && have_mid); ++k) {
        const Cipher c = skewed(k);
        const int it = run(pk, ek, c, 0x5EED0A20ULL + k).iterations;
        if (it == 1 && !have_one) { cases.push_back({"skew_one", c, true}); have_one = true; }
        if (it >= 3 && it <= 5 && !have_mid) { cases.push_back({"skew_mid", c, true}); have_mid = true; }
    }
    {
        Cipher c = fresh;
        for (Edge& e : c.E) for (uint64_t& w : e.s.w) w = 0;
        cases.push_back({"zero_sigma", c, true});
        Cipher d = fresh;   // every edge twice: merged, sigma XOR 0, doubled weights
        d.E.insert(d.E.end(), fresh.E.begin(), fresh.E.end());
        cases.push_back({"doubled", d, true});
    }
    cases.push_back({"product", read_ct_one(ref + "/pair0_mul.ct", prm.m_bits), false});
    if (!have_one || !have_mid) { std::fprintf(stderr, "no skew with 1 / 3..5 iterations\n"); return 1; }

    std::ostringstream js;
    js << "{\n  \"canon_tag\": " << pk.canon_tag << ",\n  \"pool\": " << ek.zero_pool.size() << ",\n  \"cases\": [\n";
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case& k = cases[i];
        const Result r = run(pk, ek, k.in, 0x5EED0B00ULL + i);
        if (k.sigma) write_ct(dir + "/" + k.name + "_in.ct", {k.in}, true);
        write_ct(dir + "/" + k.name + "_out.ct", {r.out}, k.sigma);
        const auto cm = commit_ct(pk, r.out);
        js << "    {\"name\": \"" << k.name << "\", \"sigma\": " << (k.sigma ? "true" : "false") << ", \"in_edges\": "
           << k.in.E.size() << ", \"in_layers\": " << k.in.L.size() << ", \"iterations\": " << r.iterations
           << ", \"out_edges\": " << r.out.E.size() << ", \"out_layers\": " << r.out.L.size()
           << ", \"density_in\": " << sigma_density(pk, k.in) << ", \"draws\": [";
        for (size_t d = 0; d < r.draws.size(); ++d) js << (d ? ", " : "") << r.draws[d];
        js << "], \"commit\": \"" << hex(cm.data(), 32) << "\"}" << (i + 1 < cases.size() ? "," : "") << "\n";
        std::printf("%-10s in %zu/%zu -> out %zu/%zu, %d iterations\n", k.name.c_str(), k.in.L.size(), k.in.E.size(),
                    r.out.L.size(), r.out.E.size(), r.iterations);
    }
    js << "  ]\n}\n";
    std::ofstream(dir + "/manifest.json") << js.str();
    return 0;
}
