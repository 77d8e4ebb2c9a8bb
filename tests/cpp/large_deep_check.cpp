// large_deep_check.cpp — csrc/large_plan.hpp for deep pairs (Lc = |A.L| + |B.L| + |A.L||B.L| above
// kLargeLayersMax, accepted under a raised layer limit) without a GPU: the limit argument of
// build_large_desc, the scratch layout of a deep pair, and the cut that keeps deep and ordinary pairs in
// sub-batches of their own. Host code only; built with ASan + UBSan by tests/cpp/Makefile.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "large_plan.hpp"

using namespace pvhip;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            ++g_failed;                                                              \
        }                                                                            \
    } while (0)

struct span {
    const char* name;
    uint64_t off, len;
};

// every region of a pair on the full (non-direct) layout with the sizes common.hpp documents
std::vector<span> regions(const large_desc& d) {
    const uint64_t LA = d.LA, LB = d.LB, nA = d.nA, nB = d.nB;
    const uint64_t hcap = d.g_head == kNoGrp && !d.iblk ? 1ull << d.hbits : 0;
    return {{"cnt", d.o_cnt, kCntWords},     {"hkey", d.o_hkey, 2 * hcap},  {"hhead", d.o_hhead, hcap},
            {"bmask", d.o_bmask, 2 * d.nblk}, {"used", d.o_used, d.Lc},      {"tkey", d.o_tkey, d.S},
            {"lstA", d.o_lstA, 2 * LA + nA}, {"lstB", d.o_lstB, 2 * LB + nB}, {"neA", d.o_neA, LA},
            {"neB", d.o_neB, LB},            {"defer", d.o_defer, LB <= kLaMaxLB ? LA * LB : 0},
            {"info", d.o_info, d.S},         {"sums", d.o_sums, 8 * d.S},   {"nxt", d.o_nxt, hcap ? d.S : 0},
            {"tb", d.o_tb, d.S},             {"within", d.o_within, d.S},   {"etot", d.o_etot, d.S},
            {"cpos", d.o_cpos, d.S},         {"order", d.o_order, d.capE},  {"hpos", d.o_hpos, d.capE}};
}

// every region inside [base, base + words) and no two overlapping
void check_regions(const large_desc& d, uint64_t base, uint64_t words, const char* what) {
    std::vector<span> a = regions(d);
    std::sort(a.begin(), a.end(), [](const span& x, const span& y) { return x.off != y.off ? x.off < y.off : x.len < y.len; });
    uint64_t end = base;
    for (const span& x : a) {
        if (x.off < end || x.off + x.len > base + words) {
            std::printf("FAILED %s: region %s [%llu, +%llu) against end %llu, words %llu\n", what, x.name,
                        (unsigned long long)x.off, (unsigned long long)x.len, (unsigned long long)end,
                        (unsigned long long)(base + words));
            ++g_failed;
        }
        end = std::max(end, x.off + x.len);
    }
    // the zeroed block covers cnt through used: the deep lists kernels count in used[0, LA + LB)
    CHECK(d.o_zero == d.o_cnt && d.o_zero + d.zero_words == d.o_used + d.Lc);
    CHECK((uint64_t)d.LA + d.LB <= d.Lc);
}

// (LA, LB, nA, nB): deep shapes of the GPU tests and their transposes
struct shape {
    uint64_t LA, LB, nA, nB;
};
const shape kDeep[] = {{1, 8192, 10, 10},   {8192, 1, 10, 10},   {33000, 1, 300, 5}, {70000, 1, 300, 5},
                       {1, 70000, 5, 300},  {128, 128, 400, 400}, {6000, 2, 500, 4},  {5462, 2, 327720, 40}};

void check_limit() {
    static_assert(sizeof(large_desc) == 352, "large_desc keeps its size: the deep kernels reuse existing scratch");
    CHECK(kLargeLayersMax == PVAC_LAYER_LIMIT_DEFAULT && PVAC_LAYER_LIMIT_MAX == (1u << 24));
    large_desc d;
    std::string why;
    // (1, 8192): Lc = 16,385, refused at the default limit with today's message, accepted at 16,385
    CHECK(build_large_desc(d, 3, 1, 8192, 10, 10, 7, why) == PVAC_ENOSYS);
    CHECK(why == "ct_mul: more than 16384 layers before compaction in one pair");
    why.clear();
    CHECK(build_large_desc(d, 3, 1, 8192, 10, 10, 7, why, false, false, kLargeLayersMax) == PVAC_ENOSYS && !why.empty());
    why.clear();
    CHECK(build_large_desc(d, 3, 1, 8192, 10, 10, 7, why, false, false, 16385) == PVAC_OK && why.empty());
    CHECK(d.Lc == 16385 && is_deep(d) && d.iblk == 0 && d.direct == 0 && d.g_head == kNoGrp && d.g_next == kNoGrp);
    // static groups and the direct mode asked for: a deep pair takes neither
    large_desc e;
    CHECK(build_large_desc(e, 3, 1, 8192, 10, 10, 7, why, true, true, 16385) == PVAC_OK);
    CHECK(e.iblk == 0 && e.direct == 0 && std::memcmp(&d, &e, sizeof d) == 0);
    // the limit is the pair's Lc: (128, 128) has 16,640
    CHECK(build_large_desc(e, 0, 128, 128, 400, 400, 7, why, false, false, 16385) == PVAC_ENOSYS);
    CHECK(why == "ct_mul: more than 16385 layers before compaction in one pair");
    CHECK(build_large_desc(e, 0, 128, 128, 400, 400, 7, why, false, false, 16640) == PVAC_OK && is_deep(e));
    // (4, 3276): Lc = 16,384 is an ordinary pair at any limit
    CHECK(build_large_desc(e, 0, 4, 3276, 10, 10, 7, why, false, false, PVAC_LAYER_LIMIT_MAX) == PVAC_OK && !is_deep(e));
    // the other bounds hold at any limit
    CHECK(build_large_desc(e, 0, 1u << 12, 1u << 12, 10, 10, 337, why, false, false, PVAC_LAYER_LIMIT_MAX) == PVAC_ENOSYS);
    CHECK(why == "ct_mul: more than 16777216 layers before compaction in one pair");
    CHECK(build_large_desc(e, 0, 3000, 3000, 10, 10, 337, why, false, false, PVAC_LAYER_LIMIT_MAX) == PVAC_ENOSYS);
    CHECK(why == "ct_mul: key space |A.L||B.L|B >= 2^31");
    CHECK(build_large_desc(e, 0, 1, 70000, 65536, 65536, 7, why, false, false, PVAC_LAYER_LIMIT_MAX) == PVAC_ENOSYS);
    CHECK(why == "ct_mul: |A.E||B.E| >= 2^32 products in one pair");
}

void check_layouts() {
    for (const shape& h : kDeep)
        for (uint32_t Bm : {7u, 337u}) {
            large_desc d;
            std::string why;
            const int rc = build_large_desc(d, 1, h.LA, h.LB, h.nA, h.nB, Bm, why, true, true, PVAC_LAYER_LIMIT_MAX);
            if (h.LA * h.LB * Bm >= (1ull << 31)) {
                CHECK(rc == PVAC_ENOSYS);
                continue;
            }
            CHECK(rc == PVAC_OK && is_deep(d) && d.iblk == 0 && d.direct == 0);
            check_regions(d, 0, d.words, "deep layout");
            large_desc r = d;
            rebase_desc(r, 0x1234560ull);
            check_regions(r, 0x1234560ull, d.words, "deep layout, rebased");
            CHECK(r.words == d.words && r.zero_words == d.zero_words);
        }
}

// ---------------------------------------------------------------- cuts
struct item {
    uint64_t LA, LB, nA, nB;
    bool sg;   // ordinary pairs: built with static groups (as the runtime rebuilds them), g_head set
};

std::vector<large_desc> make_set(const std::vector<item>& it, bool with_limit, bool allow_direct = true) {
    std::vector<large_desc> s(it.size());
    for (size_t k = 0; k < it.size(); ++k) {
        std::string why;
        const item& h = it[k];
        const int rc = with_limit ? build_large_desc(s[k], 3 * k + 1, h.LA, h.LB, h.nA, h.nB, 7, why, h.sg, h.sg && allow_direct, 1u << 20)
                                  : build_large_desc(s[k], 3 * k + 1, h.LA, h.LB, h.nA, h.nB, 7, why, h.sg, h.sg && allow_direct);
        CHECK(rc == PVAC_OK);
        if (h.sg && !is_deep(s[k])) {
            s[k].g_head = 1000 * k;
            s[k].g_next = 1000 * k + s[k].S;
        }
    }
    return s;
}

bool same(const sub_batch& x, const sub_batch& y) {
    return x.desc.size() == y.desc.size() && x.sel == y.sel && x.words == y.words && x.end == y.end &&
           x.n_iblk == y.n_iblk && x.n_direct == y.n_direct &&
           std::memcmp(x.desc.data(), y.desc.data(), x.desc.size() * sizeof(large_desc)) == 0 &&
           std::memcmp(&x.sizing, &y.sizing, sizeof x.sizing) == 0;
}

void check_cuts() {
    // ordinary pairs only: the limit argument changes neither the descriptors nor any cut
    const std::vector<item> plain = {{8, 1, 320, 20, true}, {4, 5, 200, 40, true}, {2, 2, 96, 63, true},
                                     {3, 6, 50, 70, false}, {2, 1, 96, 20, true},  {9, 2, 500, 30, true},
                                     {4, 3276, 10, 10, false}};
    const std::vector<large_desc> p0 = make_set(plain, false), p1 = make_set(plain, true);
    CHECK(std::memcmp(p0.data(), p1.data(), p0.size() * sizeof(large_desc)) == 0);
    uint64_t all = 0;
    for (const large_desc& d : p0) all += d.words;
    for (uint64_t budget : {(uint64_t)1, p0[0].words + p0[1].words, all / 2, all, (uint64_t)1 << 60})
        for (size_t i = 0; i < p0.size(); ++i) {
            sub_batch a, b;
            cut_sub_batch(p0, i, budget, a);
            cut_sub_batch(p1, i, budget, b);
            CHECK(same(a, b) && a.sizing.deep == 0);
            for (size_t k = 0; k < a.sel.size(); ++k)   // the products classes as they were
                CHECK((a.desc[a.sel[k]].LB <= kLaMaxLB) == (k < a.sizing.n_la));
        }
    // deep and ordinary pairs interleaved: a sub-batch ends where deepness changes, whatever the budget
    const std::vector<item> mixed = {{8, 1, 320, 20, true},    {1, 8192, 10, 10, false}, {8192, 1, 10, 10, false},
                                     {2, 2, 96, 63, true},     {3, 6, 50, 70, false},    {70000, 1, 300, 5, false},
                                     {128, 128, 400, 400, false}, {6000, 2, 500, 4, false}, {2, 1, 96, 20, true},
                                     {1, 70000, 5, 300, false}};
    const std::vector<large_desc> m = make_set(mixed, true, false);   // (full layouts: regions() knows those)
    const size_t ends[] = {1, 3, 5, 8, 9, 10};   // with room for everything
    for (uint64_t budget : {(uint64_t)1, (uint64_t)1 << 22, (uint64_t)1 << 60}) {
        size_t i = 0, cuts = 0;
        sub_batch sb;
        while (i < m.size()) {
            cut_sub_batch(m, i, budget, sb);
            const mul_large_args& a = sb.sizing;
            CHECK(sb.end > i && sb.end <= m.size() && sb.desc.size() == sb.end - i && a.nl == sb.end - i);
            const bool deep = is_deep(m[i]);
            CHECK(a.deep == (deep ? 1u : 0u));
            uint64_t w = 0, mE = 0, mL = 0;
            for (size_t k = i; k < sb.end; ++k) {
                CHECK(is_deep(m[k]) == deep);   // never both in one sub-batch
                check_regions(sb.desc[k - i], w, m[k].words, "cut");
                w += m[k].words;
                mE = std::max<uint64_t>(mE, std::max(m[k].nA, m[k].nB));
                mL = std::max<uint64_t>(mL, m[k].Lc);
            }
            CHECK(w == sb.words && a.max_lay == mL);
            CHECK(sb.end - i == 1 || sb.words <= budget);
            if (deep) {
                // the launch of a deep sub-batch: dynamic chains only, the lists kernels' edge grid
                CHECK(a.any_dyn == 1 && a.all_iblk == 0 && a.any_direct == 0 && a.all_direct == 0 && sb.n_iblk == 0 &&
                      sb.n_direct == 0 && a.max_nA == mE);
                // products classes: A-layer-major up to 4 B layers and below 2^16 A layers (the deferred-task
                // list packs an A layer index in 16 bits), one workgroup per task otherwise
                for (size_t k = 0; k < sb.sel.size(); ++k) {
                    const large_desc& d = sb.desc[sb.sel[k]];
                    CHECK((d.LB <= kLaMaxLB && d.LA < (1u << 16)) == (k < a.n_la));
                }
            }
            if (budget == (uint64_t)1 << 60) CHECK(cuts < 6 && sb.end == ends[cuts]);
            ++cuts;
            i = sb.end;
        }
        if (budget == 1) CHECK(cuts == m.size());
    }
}

}  // namespace

int main() {
    check_limit();
    check_layouts();
    check_cuts();
    if (g_failed) {
        std::printf("large_deep_check: %d FAILED\n", g_failed);
        return 1;
    }
    std::printf("large_deep_check: ok\n");
    return 0;
}
