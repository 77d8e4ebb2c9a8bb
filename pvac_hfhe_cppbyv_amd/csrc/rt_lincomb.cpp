// rt_lincomb.cpp — ct_lincomb plan and exec: the one-pass kernels of k_lincomb.hip for the segments
// that allow it, and the reference's literal fold on ct_add_plan / _exec for the others.
#include "ctx.hpp"

using namespace pvhip;

namespace {

bool lincomb_ok(const pvac_lincomb* S) {
    if (!S) return false;
    if (!S->n) return S->n_terms == 0;
    return S->seg_off && (S->n_terms == 0 || S->term);
}

// the kernels' view of a call; the per-term arrays are slices of lincomb.terms
lincomb_args make_args(pvac_hip_ctx* c, const pvac_ct_batch& X, const pvac_lincomb& S, const pvac_ct_batch& C) {
    auto& lc = c->lincomb;
    lincomb_args a{};
    a.X = X;
    a.C = C;
    a.n = S.n;
    a.n_terms = S.n_terms;
    a.seg_off = S.seg_off;
    a.term = S.term;
    a.scale = S.scale;
    a.flags = S.flags;
    const uint64_t w = S.n_terms + 1;
    uint64_t* p = lc.terms.get();
    a.sL = p;
    a.sE = p + w;
    a.kraw = p + 2 * w;
    a.sK = p + 3 * w;
    a.mask = p + 4 * w;
    a.tseg = lc.tseg.get();
    a.troute = lc.troute.get();
    a.wg_ids = lc.wg_ids.get();
    a.remap = lc.remap.get();
    a.cls = lc.cls.get();
    a.fold_ids = lc.fold_ids.get();
    a.tile_l = lc.tile_l.get();
    a.tile_e = lc.tile_e.get();
    a.stats = c->ps.stats.get();
    a.edge_budget = c->prm.edge_budget;
    return a;
}

// sK <- exclusive scan of kraw, then the segments' classes
hipError_t scan_and_classify(pvac_hip_ctx* c, const lincomb_args& a) {
    const uint64_t w = a.n_terms + 1;
    hipError_t e = hipMemcpyAsync(a.sK, a.kraw, w * 8, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = launch_exclusive_scan_u64(a.sK, w, c->scan_scratch.get(), nullptr, c->stream);
    if (e == hipSuccess) e = launch_lincomb_classify(a, c->stream);
    return e;
}

bool sigma_mismatch(const pvac_ct_batch* X, const pvac_ct_batch* C) {
    return X->sigma && C->sigma && X->sigma_words != C->sigma_words;
}

// The fold route: acc = {}; acc = ct_add(acc, [ct_scale] X[term]) with the existing entry points on
// one-cipher views, the accumulator in two context-owned buffers, the result copied into C's slot.
// Host-driven and synchronous: the rare path.
int fold_segments(pvac_hip_ctx* c, const pvac_ct_batch* X, const pvac_lincomb* S, pvac_ct_batch* C, uint64_t n_fold) {
    auto& lc = c->lincomb;
    const bool sig = X->sigma && C->sigma;
    const uint32_t sw = X->sigma_words;
    hipError_t e = hipSuccess;
    auto down = [&](void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
    };
    auto move = [&](void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream);
    };
    auto wait = [&] {
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    };
    std::vector<uint64_t> ids(n_fold);
    down(ids.data(), lc.fold_ids.get(), n_fold * 8);
    wait();
    if (e == hipSuccess) e = lc.words.grow(8, 8);
    if (e != hipSuccess) return hip_fail(c, e, "ct_lincomb fold (ids)");
    std::sort(ids.begin(), ids.end());
    // W[0] = 0: every view's offsets; W[2 + 2 b], W[3 + 2 b]: accumulator b's counts; W[6], W[7]: a plan's offsets
    uint64_t* const W = lc.words.get();
    auto grow_set = [&](int b, uint64_t nl, uint64_t ne) {
        auto& s = lc.acc[b];
        nl = std::max<uint64_t>(nl, 1);
        ne = std::max<uint64_t>(ne, 1);
        if (e == hipSuccess) e = s.layers.grow(nl, nl);
        if (e == hipSuccess) e = s.meta.grow(ne, ne);
        if (e == hipSuccess) e = s.w_lo.grow(ne, ne);
        if (e == hipSuccess) e = s.w_hi.grow(ne, ne);
        if (e == hipSuccess && sig) e = s.sigma.grow(ne * sw, ne * sw);
    };
    auto rows_of = [&](pvac_ct_batch& v, int b) {
        auto& s = lc.acc[b];
        v.layers = s.layers.get();
        v.meta = s.meta.get();
        v.w_lo = s.w_lo.get();
        v.w_hi = s.w_hi.get();
        v.sigma = sig ? s.sigma.get() : nullptr;
        v.sigma_words = sw;
    };
    grow_set(0, 1, 1);
    grow_set(1, 1, 1);
    std::vector<uint64_t> tm, sc, shp;
    std::vector<uint32_t> fl;
    for (const uint64_t id : ids) {
        uint64_t so[2] = {0, 0}, coff[2] = {0, 0};
        down(so, S->seg_off + id, 16);
        down(&coff[0], C->l_off + id, 8);
        down(&coff[1], C->e_off + id, 8);
        wait();
        if (e != hipSuccess) break;
        const uint64_t m = so[1] - so[0];
        tm.assign(m, 0);
        sc.assign(2 * m, 0);
        fl.assign(m, PVAC_TERM_SCALE);
        down(tm.data(), S->term + so[0], m * 8);
        if (S->scale) down(sc.data(), S->scale + 2 * so[0], m * 16);
        if (S->scale && S->flags) down(fl.data(), S->flags + so[0], m * 4);
        wait();
        shp.assign(4 * m, 0);
        for (uint64_t k = 0; k < m; ++k) {
            down(&shp[4 * k], X->l_off + tm[k], 8);
            down(&shp[4 * k + 1], X->l_cnt + tm[k], 8);
            down(&shp[4 * k + 2], X->e_off + tm[k], 8);
            down(&shp[4 * k + 3], X->e_cnt + tm[k], 8);
        }
        if (e == hipSuccess) e = hipMemsetAsync(W, 0, 8 * 8, c->stream);
        wait();
        if (e != hipSuccess) break;
        int cur = 0;
        for (uint64_t k = 0; k < m; ++k) {
            const uint64_t t = tm[k], xlo = shp[4 * k], xeo = shp[4 * k + 2], xE = shp[4 * k + 3];
            pvac_ct_batch Tv{};
            Tv.n = 1;
            Tv.l_off = Tv.e_off = W;
            Tv.l_cnt = X->l_cnt + t;
            Tv.e_cnt = X->e_cnt + t;
            Tv.layers = X->layers + xlo;
            Tv.meta = X->meta + xeo;
            Tv.w_lo = X->w_lo + xeo;
            Tv.w_hi = X->w_hi + xeo;
            Tv.sigma = sig ? X->sigma + xeo * sw : nullptr;
            Tv.sigma_words = sw;
            if (S->scale && (fl[k] & PVAC_TERM_SCALE) && xE) {   // ct_scale of a copy of the term's weights
                if (e == hipSuccess) e = lc.sw_lo.grow(xE, xE);
                if (e == hipSuccess) e = lc.sw_hi.grow(xE, xE);
                move(lc.sw_lo.get(), Tv.w_lo, xE * 8);
                move(lc.sw_hi.get(), Tv.w_hi, xE * 8);
                Tv.w_lo = lc.sw_lo.get();
                Tv.w_hi = lc.sw_hi.get();
                if (e == hipSuccess) e = launch_ct_scale(Tv, sc[2 * k], sc[2 * k + 1], c->stream);
            }
            if (e != hipSuccess) break;
            pvac_ct_batch Av{}, Cv{};
            Av.n = Cv.n = 1;
            Av.l_off = Av.e_off = W;
            Av.l_cnt = W + 2 + 2 * cur;
            Av.e_cnt = W + 3 + 2 * cur;
            rows_of(Av, cur);
            Cv.l_off = W + 6;
            Cv.e_off = W + 7;
            Cv.l_cnt = W + 2 + 2 * (1 - cur);
            Cv.e_cnt = W + 3 + 2 * (1 - cur);
            Cv.sigma_words = sw;
            pvac_hip_plan ap;
            int rc = pvac_hip_ct_add_plan(c, &Av, &Tv, &Cv, &ap);
            if (rc) return rc;
            grow_set(1 - cur, ap.total_layer_slots, ap.total_edge_slots);
            if (e != hipSuccess) break;
            rows_of(Cv, 1 - cur);
            const uint64_t deep0 = c->merge.deep_calls;
            rc = ct_add_exec(c, &ap, &Av, &Tv, 0, &Cv, deep_layer_bound(c->layer_limit));
            if (rc) return rc;
            c->deep_route[1] += c->merge.deep_calls - deep0;   // a running sum above kAddLdsLayers: k_ct_add_deep
            cur ^= 1;
        }
        if (e != hipSuccess) break;
        uint64_t cnt[2] = {0, 0};
        down(cnt, W + 2 + 2 * cur, 16);
        wait();
        const auto& s = lc.acc[cur];
        move(C->layers + coff[0], s.layers.get(), cnt[0] * sizeof(pvac_layer));
        move(C->meta + coff[1], s.meta.get(), cnt[1] * 8);
        move(C->w_lo + coff[1], s.w_lo.get(), cnt[1] * 8);
        move(C->w_hi + coff[1], s.w_hi.get(), cnt[1] * 8);
        if (sig) move(C->sigma + coff[1] * sw, s.sigma.get(), cnt[1] * sw * 8);
        move(C->l_cnt + id, W + 2 + 2 * cur, 8);
        move(C->e_cnt + id, W + 3 + 2 * cur, 8);
        wait();   // the accumulators are the next segment's
        if (e != hipSuccess) break;
    }
    return hip_fail(c, e, "ct_lincomb fold");
}

}  // namespace

extern "C" {

int pvac_hip_ct_lincomb_plan(pvac_hip_ctx* c, const pvac_ct_batch* X, const pvac_lincomb* S, pvac_ct_batch* C,
                             pvac_hip_plan* plan) try {
    if (!c || !plan || !batch_ok(X) || !C || !lincomb_ok(S) || (S->n && (!C->l_off || !C->e_off)))
        return fail(c, PVAC_EINVAL, "ct_lincomb_plan: bad arguments");
    if (sigma_mismatch(X, C)) return fail(c, PVAC_EINVAL, "ct_lincomb_plan: X and C differ in sigma_words");
    std::memset(plan, 0, sizeof *plan);
    plan->kind = 6;
    plan->n_pairs = S->n;
    auto& lc = c->lincomb;
    const uint64_t n = S->n, nt = S->n_terms;
    if (!n) {
        c->ps.invalidate();
        lc.n = lc.n_terms = lc.n_wg = lc.n_deep = lc.n_fold = 0;
        C->n = 0;
        c->ps.commit(plan);
        return PVAC_OK;
    }
    if (n >= (1ull << 31) || nt >= (1ull << 31))
        return fail(c, PVAC_ENOSYS, "ct_lincomb_plan: 2^31 segments or terms, or more");
    hipError_t e = lc.terms.grow_floor(5 * (nt + 1));
    if (e == hipSuccess) e = lc.tseg.grow_floor(nt);
    if (e == hipSuccess) e = lc.troute.grow_floor(nt);
    if (e == hipSuccess) e = lc.wg_ids.grow_floor(nt);
    if (e == hipSuccess) e = lc.cls.grow_floor(n);
    if (e == hipSuccess) e = lc.fold_ids.grow_floor(n);
    if (e != hipSuccess) return hip_fail(c, e, "alloc lincomb scratch");
    int rc = ensure_scan(c, std::max(n, nt + 1));
    if (rc) return rc;
    scoped_timer timer(c, "ct_lincomb_plan");
    lincomb_args a = make_args(c, *X, *S, *C);
    plan_stats st;
    rc = plan_pass(c, n, C, false, "ct_lincomb_plan", [&] {
        hipError_t q = hipSuccess;
        if (!nt) q = hipMemsetAsync(lc.terms.get(), 0, 5 * 8, c->stream);   // the scans' closing entries
        if (q == hipSuccess) q = launch_lincomb_plan(a, c->stream);
        if (q == hipSuccess)
            q = launch_exclusive_scan2_u64(a.sL, a.sE, nt + 1, c->scan_scratch.get(), &c->ps.totals[0], &c->ps.totals[1],
                                           c->stream);
        if (q == hipSuccess) q = scan_and_classify(c, a);
        return q;
    }, st);
    if (rc) return rc;
    // nothing has been written to C yet
    if (st.n_invalid) return fail(c, PVAC_EINVAL, "ct_lincomb_plan: bad seg_off or term index");
    // the most layers of a term and of a fold-route segment: 30000 unless the context's limit was raised
    const uint32_t bound = deep_layer_bound(c->layer_limit);
    if (st.max_layers > bound)
        return fail(c, PVAC_ENOSYS, "ct_lincomb_plan: a term above " + std::to_string(bound) + " layers");
    if (st.max_na >= (1u << 31) || st.max_prod >= (1u << 31) || st.max_nb >= (1u << 31))
        return fail(c, PVAC_ENOSYS, "ct_lincomb_plan: a layer or edge count of 2^31 or more");
    uint64_t n_wg = st.n_small, n_deep = 0;
    if (st.n_small) {
        // the workgroup route: its remap tables are sized from the first read-back, and its contract
        // flags can move segments to the fold route, so the classes are taken again
        e = lc.remap.grow_floor(st.total_layers);
        a = make_args(c, *X, *S, *C);
        lincomb_args wg = a;
        const uint64_t* deep_ids = nullptr;
        if (e == hipSuccess && st.max_layers > kLinMaxLayers) {
            // a term beyond the LDS keep table: the listed terms split by route (one more read-back),
            // the deep ones closed in the slab, at the offsets the workgroup route's remaps have
            uint64_t cnt[2] = {0, 0};
            e = lc.route_ids.grow_floor(2 + 2 * nt);
            uint64_t* const R = lc.route_ids.get();
            if (e == hipSuccess) e = hipMemsetAsync(R, 0, 16, c->stream);
            if (e == hipSuccess) e = launch_lincomb_split(a, st.n_small, R, c->stream);
            if (e == hipSuccess) e = read_back(c, cnt, R, sizeof cnt);
            if (e == hipSuccess && cnt[0] + cnt[1] != st.n_small) e = hipErrorUnknown;
            n_wg = cnt[0];
            n_deep = cnt[1];
            wg.wg_ids = R + 2;
            deep_ids = R + 2 + nt;
        }
        if (e == hipSuccess) e = hipMemsetAsync(&c->ps.stats.get()->n_large, 0, 8, c->stream);
        if (e == hipSuccess) e = launch_lincomb_plan_wg(wg, n_wg, std::min(st.max_layers, kLinMaxLayers), c->stream);
        if (e == hipSuccess) e = launch_lincomb_plan_deep(a, deep_ids, n_deep, c->stream);
        if (e == hipSuccess) e = scan_and_classify(c, a);
        plan_stats st2{};
        if (e == hipSuccess) e = read_back(c, &st2, c->ps.stats.get(), sizeof st2);
        if (e != hipSuccess) return hip_fail(c, e, "ct_lincomb_plan (workgroup route)");
        st.n_large = st2.n_large;
        st.max_buckets = st2.max_buckets;
    }
    if (st.n_large && st.max_buckets > bound)
        return fail(c, PVAC_ENOSYS, "ct_lincomb_plan: a fold-route segment above " + std::to_string(bound) + " layers");
    const uint64_t tl = (st.total_layers + kLinLayerTile - 1) / kLinLayerTile + 1;
    const uint64_t te = (st.total_edges + kLinEdgeTile - 1) / kLinEdgeTile + 1;
    e = lc.tile_l.grow_floor(tl);
    if (e == hipSuccess) e = lc.tile_e.grow_floor(te);
    a = make_args(c, *X, *S, *C);
    if (e == hipSuccess) e = launch_lincomb_layout(a, st.total_layers, st.total_edges, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "ct_lincomb_plan (layout)");
    plan->total_layer_slots = st.total_layers;
    plan->total_edge_slots = st.total_edges;
    plan->n_small = n - st.n_large;
    plan->n_large = st.n_large;
    plan->max_layers = st.max_layers;
    lc.n = n;
    lc.n_terms = nt;
    lc.n_wg = n_wg;
    lc.n_deep = n_deep;
    lc.n_fold = st.n_large;
    C->n = n;
    c->ps.commit(plan);
    return PVAC_OK;
} catch (...) { return caught(c, "ct_lincomb_plan"); }

int pvac_hip_ct_lincomb_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* X, const pvac_lincomb* S,
                             pvac_ct_batch* C) try {
    if (!c || !plan || plan->kind != 6 || !batch_ok(X) || !batch_ok(C) || !lincomb_ok(S))
        return fail(c, PVAC_EINVAL, "ct_lincomb_exec: bad arguments");
    if (S->n != plan->n_pairs || C->n != S->n) return fail(c, PVAC_EINVAL, "ct_lincomb_exec: plan mismatch");
    auto& lc = c->lincomb;
    if (!c->ps.is_latest(plan) || lc.n != S->n || lc.n_terms != S->n_terms || lc.n_fold != plan->n_large)
        return fail(c, PVAC_EINVAL, "ct_lincomb_exec: plan is not this context's latest plan");
    if (!S->n) return PVAC_OK;
    if (!C->layers || !C->meta || !C->w_lo || !C->w_hi || C->meta == X->meta || C->layers == X->layers ||
        C->w_lo == X->w_lo || C->w_hi == X->w_hi || (C->sigma && C->sigma == X->sigma))
        return fail(c, PVAC_EINVAL, "ct_lincomb_exec: C needs row arrays of its own");
    if (sigma_mismatch(X, C)) return fail(c, PVAC_EINVAL, "ct_lincomb_exec: X and C differ in sigma_words");
    {
        scoped_timer timer(c, "ct_lincomb");
        const lincomb_args a = make_args(c, *X, *S, *C);
        const int rc = hip_fail(c, launch_lincomb_copy(a, plan->total_layer_slots, plan->total_edge_slots, c->stream),
                                "ct_lincomb");
        if (rc) return rc;
    }
    lc.status_n = S->n;
    lc.path[0] += plan->n_small;
    lc.path[1] += plan->n_large;
    lc.path[2] += lc.n_terms - lc.n_wg - lc.n_deep;
    lc.path[3] += lc.n_wg;
    c->deep_route[0] += lc.n_deep;
    if (!plan->n_large) return PVAC_OK;
    return fold_segments(c, X, S, C, plan->n_large);
} catch (...) { return caught(c, "ct_lincomb_exec"); }

int pvac_hip_ct_lincomb_path_count(pvac_hip_ctx* c, uint64_t out[4]) {
    if (!c || !out) return PVAC_EINVAL;
    for (int k = 0; k < 4; ++k) out[k] = c->lincomb.path[k];
    return PVAC_OK;
}

int pvac_hip_ct_lincomb_status(pvac_hip_ctx* c, uint32_t* out, size_t n) try {
    if (!c || (!out && n)) return fail(c, PVAC_EINVAL, "ct_lincomb_status: bad arguments");
    if (n != c->lincomb.status_n) return fail(c, PVAC_EINVAL, "ct_lincomb_status: n is not the last exec's");
    if (!n) return PVAC_OK;
    return hip_fail(c, hipMemcpyAsync(out, c->lincomb.cls.get(), n * 4, hipMemcpyDeviceToDevice, c->stream),
                    "ct_lincomb_status");
} catch (...) { return caught(c, "ct_lincomb_status"); }

}  // extern "C"
