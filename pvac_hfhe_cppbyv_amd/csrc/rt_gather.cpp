// rt_gather.cpp — pvac_hip_batch_gather: whole ciphers of several resident batches regrouped into one
// dense batch on the device (kernels: k_gather.hip; the work split: gather_tiles.hpp). Concat, select,
// permute, repeat and split are all this one gather.
#include "ctx.hpp"

using namespace pvhip;

namespace {

bool same_arrays(const pvac_ct_batch& a, const pvac_ct_batch& b) {
    return a.n == b.n && a.l_off == b.l_off && a.l_cnt == b.l_cnt && a.layers == b.layers && a.e_off == b.e_off &&
           a.e_cnt == b.e_cnt && a.meta == b.meta && a.w_lo == b.w_lo && a.w_hi == b.w_hi && a.sigma == b.sigma &&
           a.sigma_words == b.sigma_words;
}

// the argument rules both calls share; nullptr = fine
const char* gather_args_error(const pvac_gather* G, const pvac_ct_batch* dst) {
    if (!G || !dst) return "null arguments";
    if (G->n_src > PVAC_GATHER_MAX_SOURCES) return "more than PVAC_GATHER_MAX_SOURCES sources";
    if (G->n_src && !G->srcs) return "null source table";
    if (!G->n_src && G->m) return "output ciphers without a source";
    if (G->pick_src && !G->pick_idx) return "pick_src without pick_idx";
    if (G->pick_idx && !G->pick_src && G->n_src != 1) return "pick_idx without pick_src takes exactly one source";
    uint64_t sum = 0;
    for (uint32_t j = 0; j < G->n_src; ++j) {
        const pvac_ct_batch& S = G->srcs[j];
        if (!batch_ok(&S)) return "a source without index arrays";
        if (S.n && (!S.layers || !S.meta || !S.w_lo || !S.w_hi)) return "a source without row arrays";
        if (dst->sigma && (!S.sigma || S.sigma_words != dst->sigma_words))
            return "dst sigma needs sigma of the same width on every source";
        sum += S.n;
    }
    if (!G->pick_idx && G->m != sum) return "without picks m is the sum of the sources' ciphers";
    if (G->m && (!dst->l_off || !dst->l_cnt || !dst->e_off || !dst->e_cnt)) return "null dst index arrays";
    return nullptr;
}

// the sigma width dst may carry: the sources' common one, 0 when a source has none or they differ
uint32_t common_sigma_words(const std::vector<pvac_ct_batch>& srcs) {
    uint32_t sw = 0;
    for (const pvac_ct_batch& S : srcs) {
        if (!S.sigma || !S.sigma_words || (sw && S.sigma_words != sw)) return 0;
        sw = S.sigma_words;
    }
    return sw;
}

// the plan's arrays over its storage
void carve(uint64_t* w, uint64_t m, uint64_t*& cL, uint64_t*& cE, uint64_t*& oL, uint64_t*& oE, uint64_t*& toff, uint64_t*& toff_s,
           uint64_t*& sL, uint64_t*& sE) {
    cL = w; cE = w + m; oL = w + 2 * m; oE = w + 3 * m; toff = w + 4 * m; toff_s = w + 5 * m; sL = w + 6 * m; sE = w + 7 * m;
}

}  // namespace

extern "C" {

int pvac_hip_batch_gather_plan(pvac_hip_ctx* c, const pvac_gather* G, pvac_ct_batch* dst, uint64_t totals[2]) try {
    if (!c || !totals) return fail(c, PVAC_EINVAL, "batch_gather_plan: null arguments");
    auto& gs = c->gather;
    gs.planned = false;
    if (const char* m = gather_args_error(G, dst)) return fail(c, PVAC_EINVAL, std::string("batch_gather_plan: ") + m);
    const uint64_t m = G->m;
    if (m >= 0x7FFFFFFFull) return fail(c, PVAC_ENOSYS, "batch_gather_plan: 2^31 - 1 output ciphers or more");
    const uint32_t ns = G->n_src;
    // kept until the next plan: exec compares G with them, and the enqueued uploads may read them late
    gs.srcs.assign(G->srcs, G->srcs + ns);
    gs.first.assign(ns + 1, 0);
    for (uint32_t j = 0; j < ns; ++j) gs.first[j + 1] = gs.first[j] + gs.srcs[j].n;
    gs.sigma_words = common_sigma_words(gs.srcs);
    gs.total_layers = gs.total_edges = gs.tiles = gs.tiles_sigma = 0;
    totals[0] = totals[1] = 0;
    if (m) {
        const int rc = ensure_scan(c, m);
        if (rc) return rc;
        static_assert(sizeof(pvac_ct_batch) % 8 == 0, "descriptors are uploaded as words");
        constexpr size_t kDescWords = sizeof(pvac_ct_batch) / 8;
        hipError_t e = gs.words.grow_floor(8 * m);
        if (e == hipSuccess) e = gs.src.grow_floor(m);
        if (e == hipSuccess) e = gs.table.grow_floor((kDescWords + 1) * ns + 1);
        if (e == hipSuccess) e = gs.ctl.grow(kGatherCtlWords, kGatherCtlWords);
        if (e != hipSuccess) return hip_fail(c, e, "alloc batch_gather scratch");
        uint64_t* table = gs.table.get();
        uint64_t* first = table + kDescWords * ns;
        e = hipMemcpyAsync(table, gs.srcs.data(), sizeof(pvac_ct_batch) * ns, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(first, gs.first.data(), 8 * (ns + 1), hipMemcpyHostToDevice, c->stream);
        gather_plan_args a{};
        a.srcs = (const pvac_ct_batch*)table;
        a.first = first;
        a.n_src = ns;
        a.g = gather_geom_of(0);
        a.gs = gather_geom_of(gs.sigma_words);
        a.m = m;
        a.pick_src = G->pick_src;
        a.pick_idx = G->pick_idx;
        carve(gs.words.get(), m, a.cL, a.cE, a.oL, a.oE, a.toff, a.toff_s, a.sL, a.sE);
        if (!gs.sigma_words) a.toff_s = nullptr;
        a.src = gs.src.get();
        a.ctl = gs.ctl.get();
        if (e == hipSuccess) e = launch_gather_plan(a, *dst, c->scan_scratch.get(), c->stream);
        unsigned long long got[kGatherCtlWords] = {};
        if (e == hipSuccess) e = read_back(c, got, a.ctl, sizeof got);
        if (e != hipSuccess) return hip_fail(c, e, "batch_gather_plan");
        if (got[3]) return fail(c, PVAC_EINVAL, "batch_gather_plan: " + std::to_string(got[3]) + " picks out of range");
        gs.total_layers = got[0];
        gs.total_edges = got[1];
        gs.tiles = got[2];
        gs.tiles_sigma = got[4];
    }
    dst->n = m;
    totals[0] = gs.total_layers;
    totals[1] = gs.total_edges;
    gs.m = m;
    gs.pick_src = G->pick_src;
    gs.pick_idx = G->pick_idx;
    gs.dst_index[0] = dst->l_off;
    gs.dst_index[1] = dst->l_cnt;
    gs.dst_index[2] = dst->e_off;
    gs.dst_index[3] = dst->e_cnt;
    gs.planned = true;
    return PVAC_OK;
} catch (...) { return caught(c, "batch_gather_plan"); }

int pvac_hip_batch_gather_exec(pvac_hip_ctx* c, const pvac_gather* G, pvac_ct_batch* dst, uint64_t layer_cap,
                               uint64_t edge_cap) try {
    if (!c) return PVAC_EINVAL;
    auto& gs = c->gather;
    if (const char* m = gather_args_error(G, dst)) return fail(c, PVAC_EINVAL, std::string("batch_gather_exec: ") + m);
    bool same = gs.planned && gs.m == G->m && gs.srcs.size() == G->n_src && gs.pick_src == G->pick_src &&
                gs.pick_idx == G->pick_idx && gs.dst_index[0] == dst->l_off && gs.dst_index[1] == dst->l_cnt &&
                gs.dst_index[2] == dst->e_off && gs.dst_index[3] == dst->e_cnt;
    for (uint32_t j = 0; same && j < G->n_src; ++j) same = same_arrays(gs.srcs[j], G->srcs[j]);
    if (!same) return fail(c, PVAC_EINVAL, "batch_gather_exec: not this context's latest gather plan of G and dst");
    if (gs.total_layers > layer_cap || gs.total_edges > edge_cap)
        return fail(c, PVAC_ENOMEM, "batch_gather_exec: layer_cap or edge_cap is too small");
    const uint64_t m = gs.m;
    if (!m) return PVAC_OK;
    if ((gs.total_layers && !dst->layers) || (gs.total_edges && (!dst->meta || !dst->w_lo || !dst->w_hi)))
        return fail(c, PVAC_EINVAL, "batch_gather_exec: null dst row arrays");
    // dst->sigma passed gather_args_error, so its width is the sources' common one: the plan's
    const uint32_t sw = dst->sigma ? dst->sigma_words : 0u;
    gather_exec_args a{};
    a.srcs = (const pvac_ct_batch*)gs.table.get();
    a.dst = *dst;
    uint64_t *cL, *cE, *oL, *oE, *toff, *toff_s, *sL, *sE;
    carve(gs.words.get(), m, cL, cE, oL, oE, toff, toff_s, sL, sE);
    a.cL = cL; a.cE = cE; a.oL = oL; a.oE = oE; a.sL = sL; a.sE = sE;
    a.toff = sw ? toff_s : toff;
    a.src = gs.src.get();
    a.m = m;
    a.ntiles = sw ? gs.tiles_sigma : gs.tiles;
    a.g = gather_geom_of(sw);
    bool wide = false;
    if (sw) {
        uint64_t bits = (uintptr_t)dst->sigma;
        for (const pvac_ct_batch& S : gs.srcs) bits |= (uintptr_t)S.sigma;
        wide = gather_sigma_wide(sw, bits);
    }
    scoped_timer t(c, "batch_gather");
    const int rc = hip_fail(c, launch_gather_rows(a, wide, c->num_cus, c->stream), "batch_gather_exec");
    if (!rc) {
        gs.path[wide ? 0 : 1]++;
        gs.path[2] += a.ntiles;
        gs.path[3] += m;
    }
    return rc;
} catch (...) { return caught(c, "batch_gather_exec"); }

int pvac_hip_batch_gather_path_count(pvac_hip_ctx* c, uint64_t out[4]) {
    if (!c || !out) return PVAC_EINVAL;
    for (int k = 0; k < 4; ++k) out[k] = c->gather.path[k];
    return PVAC_OK;
}

int pvac_hip_batch_gather_tile(uint32_t sigma_words, uint32_t out[2]) {
    if (!out) return PVAC_EINVAL;
    const gather_geom g = gather_geom_of(sigma_words);
    out[0] = g.ept;
    out[1] = g.lpt;
    return PVAC_OK;
}

}  // extern "C"
