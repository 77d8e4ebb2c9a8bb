// mint_lincomb.cpp — TEST INFRASTRUCTURE ONLY: mints tests/golden/lincomb/ with the unmodified
// reference's ct_add / ct_scale (ops/arithmetic.hpp:12-37) and commit_ct (ops/commit.hpp). The engine
// never links, loads or calls it.
//
//   g++ -std=c++17 -O2 -march=native -w -I<reference>/include -pthread \
//       -o oracle/_ref/mint_lincomb tools/mint_lincomb.cpp
//   oracle/_ref/mint_lincomb tests/golden/ref tests/golden/lincomb
//
// No key is generated: ct_add, ct_scale and commit_ct read only pk.prm, pk.canon_tag and pk.H_digest,
// and the last two are taken from <golden ref>/manifest.json. Every case is the literal fold
//     acc = Cipher{}; for k: t = X[term[k]]; if (flags[k] & 1) t = ct_scale(pk, t, scale[k]); acc = ct_add(pk, acc, t);
// over existing <golden ref>/*.ct inputs (and the one input invented here, unused_in.ct).
//
// Output: manifest.json with, per case, the terms (paths under tests/golden), scales as (lo, hi) words,
// flags, edge_budget, sigma on / off, the output's layer and edge counts and its commit_ct (a
// weights-only case commits with every edge's nbits = 0); and unused_in.ct.
#include <pvac/pvac.hpp>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace pvac;

static void put32(std::ostream& o, uint32_t x) { o.write((const char*)&x, 4); }
static void put64(std::ostream& o, uint64_t x) { o.write((const char*)&x, 8); }

// the reference's .ct layout (tests/add.cpp:22-155)
static void write_ct(const std::string& path, const std::vector<Cipher>& cts) {
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
            put32(o, (uint32_t)e.s.nbits);
            for (size_t i = 0; i < (e.s.nbits + 63) / 64; ++i) put64(o, e.s.w[i]);
        }
    }
}

// the first cipher of a file; with_sigma = false drops the sigmas (every edge's nbits = 0)
static Cipher read_ct_one(const std::string& path, bool with_sigma) {
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
        if (with_sigma && !nbits) { std::fprintf(stderr, "%s carries no sigma\n", path.c_str()); std::exit(2); }
        e.s = BitVec::make(with_sigma ? nbits : 0);
        for (size_t w = 0; w < (nbits + 63) / 64; ++w) {
            const uint64_t x = g64();
            if (with_sigma) e.s.w[w] = x;
        }
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

struct Term {
    std::string path;   // under tests/golden
    bool scaled;
    Fp scale;
};
struct Case {
    std::string name;
    bool sigma;
    size_t edge_budget;
    std::vector<Term> terms;
};

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <golden ref dir> <out dir>\n", argv[0]); return 2; }
    const std::string ref = argv[1], dir = argv[2];
    PubKey pk;
    {   // canon_tag and H_digest of the fixture key
        std::ifstream f(ref + "/manifest.json");
        std::stringstream ss;
        ss << f.rdbuf();
        const std::string man = ss.str();
        const size_t a = man.find("\"canon_tag\": "), b = man.find("\"H_digest\": \"");
        if (a == std::string::npos || b == std::string::npos) { std::fprintf(stderr, "no key in %s/manifest.json\n", ref.c_str()); return 1; }
        pk.canon_tag = std::strtoull(man.c_str() + a + 13, nullptr, 10);
        for (int i = 0; i < 32; ++i) pk.H_digest[i] = (uint8_t)std::strtoul(man.substr(b + 13 + 2 * i, 2).c_str(), nullptr, 16);
    }
    const Fp one{1, 0}, pm1{~0ull - 1, ~0ull >> 1}, p{~0ull, ~0ull >> 1}, all{~0ull, ~0ull}, zero{0, 0};
    auto plain = [](const std::string& path) { return Term{path, false, Fp{0, 0}}; };
    auto scaled = [](const std::string& path, Fp s) { return Term{path, true, s}; };

    {   // the invented input: enc4 without the edges of its second layer (an unused BASE layer)
        Cipher c = read_ct_one(ref + "/enc4.ct", true);
        std::vector<Edge> keep;
        for (const Edge& e : c.E)
            if (e.layer_id != 1) keep.push_back(e);
        c.E.swap(keep);
        write_ct(dir + "/unused_in.ct", {c});
    }

    std::vector<Case> cases;
    cases.push_back({"sum3", true, 1200000, {plain("ref/enc0.ct"), plain("ref/enc1.ct"), plain("ref/enc2.ct")}});
    cases.push_back({"one", true, 1200000, {plain("ref/enc3.ct")}});
    cases.push_back({"none", true, 1200000, {}});
    cases.push_back({"poly", false, 1200000,
                     {scaled("ref/pair0_mul_w.ct", one), scaled("ref/pair1_mul_w.ct", pm1), scaled("ref/pair2_mul_w.ct", Fp{5, 0}),
                      scaled("ref/pair0_x.ct", Fp{3, 1}), plain("ref/pair1_x.ct")}});
    cases.push_back({"fullrange", false, 1200000,
                     {scaled("ref/fr0_x.ct", zero), scaled("ref/fr1_x.ct", one), scaled("ref/fr2_x.ct", p),
                      scaled("ref/fr3_x.ct", all), plain("ref/fr4_x.ct")}});
    cases.push_back({"unused", true, 1200000, {plain("lincomb/unused_in.ct"), plain("ref/enc5.ct"), plain("lincomb/unused_in.ct")}});
    cases.push_back({"chains", false, 1200000,
                     {plain("ref/chain1.ct"), plain("ref/chain2.ct"), plain("ref/chain3.ct"), scaled("ref/chainf_final.ct", pm1),
                      plain("ref/chainf_final.ct")}});
    cases.push_back({"guard", true, 100, {plain("ref/enc0.ct"), plain("ref/enc1.ct"), plain("ref/enc2.ct"), plain("ref/enc3.ct")}});

    const std::string golden = ref + "/..";
    std::ostringstream js;
    js << "{\n  \"canon_tag\": " << pk.canon_tag << ",\n  \"H_digest\": \"" << hex(pk.H_digest.data(), 32) << "\",\n  \"cases\": [\n";
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case& k = cases[i];
        pk.prm = Params{};
        pk.prm.edge_budget = k.edge_budget;
        Cipher acc;
        for (const Term& t : k.terms) {
            Cipher x = read_ct_one(golden + "/" + t.path, k.sigma);
            if (t.scaled) x = ct_scale(pk, x, t.scale);
            acc = ct_add(pk, acc, x);
        }
        const auto cm = commit_ct(pk, acc);
        js << "    {\"name\": \"" << k.name << "\", \"sigma\": " << (k.sigma ? "true" : "false") << ", \"edge_budget\": "
           << k.edge_budget << ",\n     \"terms\": [";
        for (size_t j = 0; j < k.terms.size(); ++j) js << (j ? ", " : "") << "\"" << k.terms[j].path << "\"";
        js << "],\n     \"scales\": [";
        for (size_t j = 0; j < k.terms.size(); ++j)
            js << (j ? ", " : "") << "[" << k.terms[j].scale.lo << ", " << k.terms[j].scale.hi << "]";
        js << "],\n     \"flags\": [";
        for (size_t j = 0; j < k.terms.size(); ++j) js << (j ? ", " : "") << (k.terms[j].scaled ? 1 : 0);
        js << "],\n     \"out_layers\": " << acc.L.size() << ", \"out_edges\": " << acc.E.size() << ", \"commit\": \""
           << hex(cm.data(), 32) << "\"}" << (i + 1 < cases.size() ? "," : "") << "\n";
        std::printf("%-10s %zu terms -> %zu layers, %zu edges\n", k.name.c_str(), k.terms.size(), acc.L.size(), acc.E.size());
    }
    js << "  ]\n}\n";
    std::ofstream(dir + "/manifest.json") << js.str();
    return 0;
}
