// enc_wide_check.cpp — CPU-only checks of csrc/enc_wide.hpp, the table logic of the wide encryption
// route, against the brute-force definition of compact_edges' grouping (reference ops/encrypt.hpp:39-71:
// merged edges sorted by (idx, P before M), contributors in creation order), and of its host sizing:
// draws_hint, the sub-batch cuts and the scratch layout. A stand-alone host program; tests/cpp/wide.mk
// builds it with AddressSanitizer and UBSan, tests/test_enc_wide_host.py runs it.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "enc_wide.hpp"

using namespace pvhip;

static int fails = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
            ++fails;                                              \
        }                                                         \
    } while (0)

static uint64_t sm(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// keys of npre edges over `nkeys` distinct (idx, ch) pairs drawn from B indices
static std::vector<uint32_t> seeded_keys(uint32_t npre, uint32_t B, uint32_t nkeys, uint64_t seed) {
    std::vector<uint32_t> pool;
    for (uint32_t q = 0; q < nkeys; ++q) pool.push_back((uint32_t)(sm(seed) % B) | (uint32_t)(sm(seed) & 1) << 16);
    std::vector<uint32_t> key(npre);
    for (uint32_t e = 0; e < npre; ++e) key[e] = pool[sm(seed) % pool.size()];
    return key;
}

static void check_grouping(const std::vector<uint32_t>& key, uint32_t B, const char* what) {
    const uint32_t npre = (uint32_t)key.size();
    // brute force: first occurrences by comparing with every earlier edge, ranks by counting the
    // distinct keys below, segments by collecting in creation order
    std::vector<bool> first(npre);
    for (uint32_t e = 0; e < npre; ++e) {
        first[e] = true;
        for (uint32_t q = 0; q < e; ++q) first[e] = first[e] && key[q] != key[e];
    }
    std::map<uint32_t, std::vector<uint32_t>> groups;   // ordered by sk = 2 idx + ch
    for (uint32_t e = 0; e < npre; ++e) groups[wide_sk(key[e])].push_back(e);
    std::vector<uint32_t> tab(2 * (size_t)B, 0), occ(npre + 1, 0xAAAAAAAAu), gstart(npre + 1, 0xAAAAAAAAu), ord(npre + 1, 0xAAAAAAAAu);
    const uint32_t nout = wide_group_host(key.data(), npre, B, tab.data(), occ.data(), gstart.data(), ord.data());
    CHECK(nout == groups.size());
    CHECK(occ[npre] == 0xAAAAAAAAu && gstart[npre] == 0xAAAAAAAAu && ord[npre] == 0xAAAAAAAAu);
    uint32_t firsts = 0;
    for (uint32_t e = 0; e < npre; ++e) {
        CHECK((occ[e] == 0) == first[e]);
        firsts += first[e];
    }
    CHECK(firsts == nout);
    uint32_t g = 0;
    for (const auto& kv : groups) {   // rank g = the present keys below
        uint32_t b = 0, e = 0;
        wide_segment(gstart.data(), nout, npre, g, b, e);
        CHECK(e - b == kv.second.size());
        for (uint32_t q = b; q < e && q - b < kv.second.size(); ++q) CHECK(ord[q] == kv.second[q - b]);   // creation order
        for (uint32_t q = b; q < e; ++q) CHECK(wide_sk(key[ord[q]]) == kv.first);
        ++g;
    }
    if (fails) std::printf("  in %s\n", what);
}

int main() {
    // B = 2: 300 edges on the 4 keys there are
    check_grouping(seeded_keys(300, 2, 64, 1), 2, "B=2");
    // B = 337 at hints 125 and 400 (782 edges on 674 keys: merging forced)
    check_grouping(seeded_keys(257, 337, 257, 2), 337, "B=337 npre=257");
    check_grouping(seeded_keys(782, 337, 782, 3), 337, "B=337 npre=782");
    // B = 65536: a table LDS could not hold
    check_grouping(seeded_keys(300, 65536, 300, 4), 65536, "B=65536");
    check_grouping(std::vector<uint32_t>(500, 336u | 1u << 16), 337, "one key");       // every edge on the last key
    check_grouping(seeded_keys(8, 337, 8, 5), 337, "no noise groups");                 // the signal alone
    {   // the highest and the lowest key together
        std::vector<uint32_t> k = {65535u | 1u << 16, 0u, 65535u | 1u << 16, 0u, 65535u};
        check_grouping(k, 65536, "extremes");
    }

    // draws_hint: up to 256 edges exactly what it was, above a slack that grows with the plan
    CHECK(enc_npre(68, 37) == 255 && enc_npre(69, 37) == 257);
    CHECK(enc_draws_hint(68, 37, 337, 1) == 2 + 16 + 14 + 255 + 68 * 5 + 37 * 10 + 255 + 32);
    CHECK(enc_draws_hint(68, 37, 337, 2) == 2 + 2 * (2 + 16 + 14 + 255 + 68 * 5 + 37 * 10 + 255) + 64);
    CHECK(enc_draws_hint(0, 0, 337, 1) == 2 + 16 + 14 + 8 + 8 + 32);
    CHECK(enc_half_slack(69, 37, 337) == 146);
    CHECK(enc_draws_hint(69, 37, 337, 1) == enc_half_draws(69, 37) + 146);
    CHECK(enc_draws_hint(69, 37, 337, 2) == 2 + 2 * enc_half_draws(69, 37) + 292);
    CHECK(enc_half_slack(2150, 1172, 337) == 146);                       // hint 4096: 6 mu = 102
    CHECK(enc_half_slack(100000, 100000, 337) == (6 * 400028ull + 336) / 337);
    CHECK(enc_half_slack(1000, 1000, 2) == 6 * 4028 / 2);

    // sub-batch cuts: consecutive, within the budget, an item above it alone
    {
        const uint64_t pe[] = {100, 300, 500, 1200, 50, 50, 900, 1};
        std::vector<size_t> cuts;
        enc_cuts(pe, 8, 900, cuts);
        const std::vector<size_t> want = {0, 3, 4, 6, 7, 8};   // {100,300,500} {1200} {50,50} {900} {1}
        CHECK(cuts == want);
        enc_cuts(pe, 8, 1ull << 22, cuts);
        CHECK(cuts == (std::vector<size_t>{0, 8}));
        enc_cuts(pe, 8, 1, cuts);
        CHECK(cuts.size() == 9);
        enc_cuts(pe, 0, 900, cuts);
        CHECK(cuts == (std::vector<size_t>{0}));
    }

    // scratch layout: aligned, in order, nothing overlaps, the parts a sub-batch lacks take nothing
    {
        enc_sub_shape s;
        s.n = 5; s.n_narrow = 2; s.n_wide = 3; s.halves = 7; s.pe = 3000; s.cores = 4000;
        s.work_narrow = 40; s.work_wide = 1200; s.fin = 200; s.B = 337; s.sigma_words = 128;
        const enc_sub_layout L = enc_sub_layout_of(s, 64, 72, 32, 40);
        const uint64_t offs[] = {L.recs_narrow, L.recs_wide, L.nid, L.wid, L.perm, L.work_narrow, L.work_wide, L.fin, L.half_item,
                                 L.up_bytes, L.req, L.core, L.pre_idx, L.tmp_idx, L.tmp_status, L.lay, L.e, L.key, L.grp, L.occ,
                                 L.tab, L.dlast, L.sig, L.total};
        for (size_t q = 0; q + 1 < sizeof offs / sizeof *offs; ++q) CHECK(offs[q] % 256 == 0 && offs[q] <= offs[q + 1]);
        CHECK(L.hdr == L.up_bytes);
        CHECK(L.key - L.e >= 3000 * 48 && L.grp - L.key >= 3000 * 4 && L.occ - L.grp >= 3000 * 2 && L.tab - L.occ >= 3000 * 16);
        CHECK(L.dlast - L.tab >= 3ull * 2 * 674 * 4 && L.sig - L.dlast >= 7 * 16 && L.total - L.sig >= 3000ull * 1024);
        // per pre-merge edge: the sigma row and 70 bytes of rows
        CHECK(L.total - L.e < 3000ull * (1024 + 70) + 3ull * 2 * 674 * 4 + 7 * 16 + 8 * 256);
        s.n_wide = 0; s.n_narrow = 5; s.work_wide = 0; s.fin = 0; s.sigma_words = 0;
        const enc_sub_layout N = enc_sub_layout_of(s, 64, 72, 32, 40);
        CHECK(N.tab == N.occ && N.dlast == N.tab && N.sig == N.dlast && N.total == N.sig);
    }

    if (fails) {
        std::printf("enc_wide_check: %d failed\n", fails);
        return 1;
    }
    std::printf("enc_wide_check: ok\n");
    return 0;
}
