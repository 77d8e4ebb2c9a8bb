// rt_recrypt.cpp — ct_recrypt and its parts: set_ubk, sigma_popcount, ubk_apply, compact (plan / exec)
// and the host-driven recrypt loop over them.
#include "ctx.hpp"

using namespace pvhip;

extern "C" {

int pvac_hip_ctx_set_ubk(pvac_hip_ctx* c, const int32_t* inv, uint32_t m_bits) try {
    if (!c || !inv) return fail(c, PVAC_EINVAL, "set_ubk: arguments");
    if (m_bits != c->prm.m_bits) return fail(c, PVAC_EINVAL, "set_ubk: m_bits is not the context's");
    // the kernel gathers: output bit j = input bit perm[j], perm[inv[src]] = src
    std::vector<uint32_t> perm(m_bits, 0xFFFFFFFFu);
    for (uint32_t s = 0; s < m_bits; ++s) {
        const int32_t j = inv[s];
        if (j < 0 || (uint32_t)j >= m_bits || perm[j] != 0xFFFFFFFFu)
            return fail(c, PVAC_EINVAL, "set_ubk: inv is not a permutation of [0, m_bits)");
        perm[j] = s;
    }
    hipError_t e = hipStreamSynchronize(c->stream);   // an earlier ubk_apply may still read the table
    if (e == hipSuccess) e = c->recrypt.ubk_perm.grow(m_bits, m_bits);
    if (e == hipSuccess) e = hipMemcpy(c->recrypt.ubk_perm.get(), perm.data(), (size_t)m_bits * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(c, e, "set_ubk");
    c->recrypt.have_ubk = true;
    return PVAC_OK;
} catch (...) { return caught(c, "set_ubk"); }

namespace {

// compact's plan: the class of every cipher of X (pair_class), the merge set of the ciphers above
// the LDS bound (with C's edge offsets) and, with `scan`, C's offsets as the scans of X's counts
int compact_classify(pvac_hip_ctx* c, const pvac_ct_batch* X, pvac_ct_batch* C, bool scan, pvac_hip_plan* plan) {
    std::memset(plan, 0, sizeof *plan);
    plan->kind = 5;
    plan->n_pairs = X->n;
    c->merge.set.clear();
    if (!X->n) return PVAC_OK;
    if (X->n > 0x7FFFFFFFull) return fail(c, PVAC_ENOSYS, "compact: more than 2^31 - 1 ciphers");
    pvac_ct_batch Cw = *C;
    if (!scan) Cw.l_off = Cw.e_off = nullptr;
    plan_stats st;
    int rc = plan_pass(c, X->n, C, scan, "compact_plan", [&] {
        return launch_compact_plan(*X, Cw, c->prm.B, c->ps.pair_class.get(), c->ps.large_ids.get(), c->ps.stats.get(), c->stream);
    }, st);
    if (rc) return rc;
    plan_fill(plan, X->n, st);
    if (st.n_large) {
        // the merge kernel keeps its layer table in global scratch, so the layer bound is ct_add's
        const uint32_t bound = deep_layer_bound(c->layer_limit);
        const std::string limit_msg =
            "compact_plan: a cipher beyond " + std::to_string(bound) + " layers, 2^31 edges or 2^32 keys";
        rc = merge_gather(
            c, st.n_large,
            [&](uint64_t* out) { return launch_compact_gather(*X, *C, c->ps.large_ids.get(), st.n_large, out, c->stream); },
            [&](const uint64_t* o, merge_pair_info& m) {
                m.pair = o[0];
                m.LA = m.L = (uint32_t)o[1];
                m.nA = o[2];
                m.nB = 0;
                m.aeo = o[3];
                m.beo = 0;
                m.ceo = o[4];
                return !(o[1] > bound || m.nA >= (1ull << 31) || o[1] * c->prm.B * 2 >= 0xFFFFFFFFull);
            },
            "compact_plan (merge)", limit_msg.c_str());
        if (rc) return rc;
    }
    c->ps.commit(plan);
    return PVAC_OK;
}

int compact_execute(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* X, pvac_ct_batch* C) {
    if (!X->n) return PVAC_OK;
    if (!c->ps.is_latest(plan) || plan->n_large != c->merge.set.size())
        return fail(c, PVAC_EINVAL, "compact_exec: plan is not this context's latest plan");
    scoped_timer t(c, "compact");
    if (plan->n_small) {
        const int rc = hip_fail(c,
                                launch_compact_small(*X, *C, c->ps.pair_class.get(), c->prm.B, c->prm.m_bits, plan->max_keys,
                                                     c->stream),
                                "compact");
        if (rc) return rc;
        c->recrypt.compact_path[0] += plan->n_small;
    }
    if (!plan->n_large) return PVAC_OK;
    // the merge path of ct_add's guard_budget (k_add_merge.hip), one cipher at a time, with an empty B
    hipError_t e = c->merge.zero_n.grow(X->n, std::max<size_t>(X->n, 1024));
    if (e == hipSuccess) e = hipMemsetAsync(c->merge.zero_n.get(), 0, X->n * 8, c->stream);
    if (e == hipSuccess) e = c->merge.counters.grow(2, 2);
    if (e != hipSuccess) return hip_fail(c, e, "alloc compact merge");
    pvac_ct_batch Bz = *X;
    Bz.l_off = Bz.l_cnt = Bz.e_off = Bz.e_cnt = c->merge.zero_n.get();
    const int rc = merge_execute(c, *X, Bz, *C, 0, "compact merge");
    if (rc) return rc;
    c->recrypt.compact_path[1] += plan->n_large;
    for (const merge_pair_info& m : c->merge.set) c->deep_route[2] += m.L > kAddLdsLayers;
    return PVAC_OK;
}

}  // namespace

int pvac_hip_sigma_popcount(pvac_hip_ctx* c, const pvac_ct_batch* X, uint64_t* ones) try {
    if (!c || !batch_ok(X) || (!ones && X->n)) return fail(c, PVAC_EINVAL, "sigma_popcount: bad arguments");
    if (!X->n) return PVAC_OK;
    if (!sigma_ok(c, X)) return fail(c, PVAC_EINVAL, "sigma_popcount: X carries no sigma of m_bits");
    if (X->n > 0x7FFFFFFFull) return fail(c, PVAC_ENOSYS, "sigma_popcount: more than 2^31 - 1 ciphers");
    scoped_timer t(c, "sigma_popcount");
    return hip_fail(c, launch_sigma_popcount(*X, c->prm.m_bits, c->num_cus, (unsigned long long*)ones, c->stream),
                    "sigma_popcount");
} catch (...) { return caught(c, "sigma_popcount"); }

int pvac_hip_ubk_apply(pvac_hip_ctx* c, pvac_ct_batch* X, const uint32_t* active) try {
    if (!c || !batch_ok(X)) return fail(c, PVAC_EINVAL, "ubk_apply: bad arguments");
    if (!c->recrypt.have_ubk) return fail(c, PVAC_EINVAL, "ubk_apply: set_ubk first");
    if (!X->n) return PVAC_OK;
    if (!sigma_ok(c, X)) return fail(c, PVAC_EINVAL, "ubk_apply: X carries no sigma of m_bits");
    if (ubk_apply_lds_bytes(c->prm.m_bits) > 64 * 1024) return fail(c, PVAC_ENOSYS, "ubk_apply: m_bits beyond the LDS table");
    scoped_timer t(c, "ubk_apply");
    return hip_fail(c, launch_ubk_apply(*X, c->recrypt.ubk_perm.get(), c->prm.m_bits, active, c->num_cus, c->stream), "ubk_apply");
} catch (...) { return caught(c, "ubk_apply"); }

int pvac_hip_compact_plan(pvac_hip_ctx* c, const pvac_ct_batch* X, pvac_ct_batch* C, pvac_hip_plan* plan) try {
    if (!c || !plan || !batch_ok(X) || !C || (X->n && (!C->l_off || !C->e_off)))
        return fail(c, PVAC_EINVAL, "compact_plan: bad arguments");
    if (X->n && !sigma_ok(c, X)) return fail(c, PVAC_EINVAL, "compact_plan: X carries no sigma of m_bits");
    C->n = X->n;
    return compact_classify(c, X, C, true, plan);
} catch (...) { return caught(c, "compact_plan"); }

int pvac_hip_compact_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* X, pvac_ct_batch* C) try {
    if (!c || !plan || plan->kind != 5 || !batch_ok(X) || !batch_ok(C))
        return fail(c, PVAC_EINVAL, "compact_exec: bad arguments");
    if (X->n != plan->n_pairs || C->n != plan->n_pairs) return fail(c, PVAC_EINVAL, "compact_exec: plan mismatch");
    if (!X->n) return PVAC_OK;
    if (!sigma_ok(c, X) || !sigma_ok(c, C)) return fail(c, PVAC_EINVAL, "compact_exec: X and C must carry sigma of m_bits");
    if (!C->layers || !C->meta || !C->w_lo || !C->w_hi || C->meta == X->meta || C->sigma == X->sigma ||
        C->layers == X->layers)
        return fail(c, PVAC_EINVAL, "compact_exec: C needs row arrays of its own");
    return compact_execute(c, plan, X, C);
} catch (...) { return caught(c, "compact_exec"); }

int pvac_hip_compact_path_count(pvac_hip_ctx* c, uint64_t out[2]) {
    if (!c || !out) return PVAC_EINVAL;
    out[0] = c->recrypt.compact_path[0];
    out[1] = c->recrypt.compact_path[1];
    return PVAC_OK;
}

int pvac_hip_ct_recrypt_plan(pvac_hip_ctx* c, const pvac_ct_batch* X, const pvac_ct_batch* pool, pvac_ct_batch* C,
                             pvac_hip_plan* plan) try {
    if (!c || !plan || !batch_ok(X) || !batch_ok(pool) || !C || (X->n && (!C->l_off || !C->e_off)))
        return fail(c, PVAC_EINVAL, "ct_recrypt_plan: bad arguments");
    std::memset(plan, 0, sizeof *plan);
    plan->kind = 4;
    plan->n_pairs = X->n;
    C->n = X->n;
    if (!X->n) return PVAC_OK;
    int rc = ensure_scan(c, X->n);
    if (rc) return rc;
    // the pool is a handful of ciphers: its largest member from a host copy of the counts
    std::vector<uint64_t> pc(2 * pool->n);
    hipError_t e = hipSuccess;
    if (pool->n) {
        e = hipMemcpyAsync(pc.data(), pool->l_cnt, pool->n * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(pc.data() + pool->n, pool->e_cnt, pool->n * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    uint64_t max_pl = 0, max_pe = 0;
    for (uint64_t k = 0; k < pool->n; ++k) {
        max_pl = std::max(max_pl, pc[k]);
        max_pe = std::max(max_pe, pc[pool->n + k]);
    }
    if (e == hipSuccess) e = launch_recrypt_plan(*X, max_pl, max_pe, *C, c->stream);
    if (e == hipSuccess)
        e = launch_exclusive_scan2_u64(C->l_off, C->e_off, X->n, c->scan_scratch.get(), &c->ps.totals[0], &c->ps.totals[1],
                                       c->stream);
    unsigned long long tot[2] = {0, 0};
    if (e == hipSuccess) e = read_back(c, tot, c->ps.totals, sizeof tot);
    if (e != hipSuccess) return hip_fail(c, e, "ct_recrypt_plan");
    plan->total_layer_slots = tot[0];
    plan->total_edge_slots = tot[1];
    plan->max_layers = (uint32_t)std::min<uint64_t>(max_pl, 0xFFFFFFFFu);
    plan->max_nb = (uint32_t)std::min<uint64_t>(max_pe, 0xFFFFFFFFu);
    return PVAC_OK;
} catch (...) { return caught(c, "ct_recrypt_plan"); }

int pvac_hip_ct_recrypt_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* X, const pvac_ct_batch* pool,
                             const uint64_t* picks, pvac_ct_batch* C, uint32_t* iters) try {
    if (!c || !plan || plan->kind != 4 || !batch_ok(X) || !batch_ok(pool) || !batch_ok(C))
        return fail(c, PVAC_EINVAL, "ct_recrypt_exec: bad arguments");
    const uint64_t n = X->n, pn = pool->n;
    if (n != plan->n_pairs || C->n != n) return fail(c, PVAC_EINVAL, "ct_recrypt_exec: plan mismatch");
    if (!n) return PVAC_OK;
    if (!c->recrypt.have_ubk) return fail(c, PVAC_EINVAL, "ct_recrypt_exec: set_ubk first");
    const uint32_t sw = X->sigma_words, m_bits = c->prm.m_bits;
    if (!sigma_ok(c, X) || !sigma_ok(c, C) || (pn && !sigma_ok(c, pool)))
        return fail(c, PVAC_EINVAL, "ct_recrypt_exec: X, pool and C must carry sigma of m_bits");
    if ((sw & 1u) || C->sigma_words != sw || (pn && pool->sigma_words != sw))
        return fail(c, PVAC_EINVAL, "ct_recrypt_exec: X, pool and C need one even sigma_words");
    if (!C->layers || !C->meta || !C->w_lo || !C->w_hi || C->meta == X->meta || C->sigma == X->sigma)
        return fail(c, PVAC_EINVAL, "ct_recrypt_exec: C needs row arrays of its own");
    if (pn && !picks) return fail(c, PVAC_EINVAL, "ct_recrypt_exec: picks");
    if (n > 0x7FFFFFFFull) return fail(c, PVAC_ENOSYS, "ct_recrypt_exec: more than 2^31 - 1 ciphers");
    if (ubk_apply_lds_bytes(m_bits) > 64 * 1024) return fail(c, PVAC_ENOSYS, "ct_recrypt_exec: m_bits beyond the LDS table");
    scoped_timer timer(c, "ct_recrypt");
    // the shapes of X, of the pool and of C's slots on the host: the loop below is host-driven
    std::vector<uint64_t> hx(4 * n), hp(4 * pn), hc(2 * n);
    hipError_t e = hipSuccess;
    auto down = [&](uint64_t* dst, const uint64_t* src, uint64_t k) {
        if (e == hipSuccess && k) e = hipMemcpyAsync(dst, src, k * 8, hipMemcpyDeviceToHost, c->stream);
    };
    down(&hx[0], X->l_off, n);
    down(&hx[n], X->l_cnt, n);
    down(&hx[2 * n], X->e_off, n);
    down(&hx[3 * n], X->e_cnt, n);
    down(hp.data(), pool->l_off, pn);
    down(hp.data() + pn, pool->l_cnt, pn);
    down(hp.data() + 2 * pn, pool->e_off, pn);
    down(hp.data() + 3 * pn, pool->e_cnt, pn);
    down(&hc[0], C->l_off, n);
    down(&hc[n], C->e_off, n);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    for (uint64_t k = 0; e == hipSuccess && k < pn; ++k)   // C's slots were sized for the plan's pool
        if (hp[pn + k] > plan->max_layers || hp[3 * pn + k] > plan->max_nb)
            return fail(c, PVAC_EINVAL, "ct_recrypt_exec: the pool is larger than the planned one");
    if (e == hipSuccess) e = c->recrypt.idx.grow(17 * n, 17 * std::max<uint64_t>(n, 64));
    if (e == hipSuccess) e = c->recrypt.ids.grow(n, std::max<uint64_t>(n, 64));
    if (e != hipSuccess) return hip_fail(c, e, "ct_recrypt_exec (shapes)");
    uint64_t* const R = c->recrypt.idx.get();
    auto region = [&](int k) { return R + (uint64_t)k * n; };
    // the ciphers recrypt returns verbatim (recrypt.hpp:27), and the others: the loop's first view, in X
    std::vector<uint32_t> ids, cur_id;
    std::vector<uint64_t> cur[4];
    for (uint64_t i = 0; i < n; ++i) {
        if (iters) iters[i] = 0;
        if (!pn || !hx[3 * n + i]) {
            ids.push_back((uint32_t)i);
            continue;
        }
        cur_id.push_back((uint32_t)i);
        for (int f = 0; f < 4; ++f) cur[f].push_back(hx[f * n + i]);
    }
    if (!ids.empty()) {
        e = upload_words(c, c->recrypt.ids.get(), ids.data(), ids.size() * 4);
        if (e == hipSuccess) e = launch_recrypt_copy(*X, *C, c->recrypt.ids.get(), ids.size(), m_bits, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "ct_recrypt_exec (copy)");
    }
    pvac_ct_batch base = *X;   // the arrays the current view's ciphers live in
    std::vector<uint64_t> up, ones;
    for (int it = 0; !cur_id.empty(); ++it) {
        const uint64_t m = cur_id.size();
        // the view of the ciphers still in the loop: regions 0..3
        auto view_up = [&](const std::vector<uint32_t>& sel, int first_region) {
            for (int f = 0; f < 4 && e == hipSuccess; ++f) {
                up.resize(sel.size());
                for (size_t k = 0; k < sel.size(); ++k) up[k] = cur[f][sel[k]];
                e = upload_words(c, region(first_region + f), up.data(), up.size() * 8);
            }
        };
        auto view_of = [&](const pvac_ct_batch& b, uint64_t count, int first_region) {
            pvac_ct_batch v = b;
            v.n = count;
            v.l_off = region(first_region);
            v.l_cnt = region(first_region + 1);
            v.e_off = region(first_region + 2);
            v.e_cnt = region(first_region + 3);
            return v;
        };
        std::vector<uint32_t> all(m), fin, cont;
        for (uint64_t k = 0; k < m; ++k) all[k] = (uint32_t)k;
        if (it < 8) {
            // sigma_needs_balance (recrypt.hpp:21-24) from the exact popcounts, in the reference's arithmetic
            view_up(all, 0);
            const pvac_ct_batch V = view_of(base, m, 0);
            if (e == hipSuccess)
                e = launch_sigma_popcount(V, m_bits, c->num_cus, (unsigned long long*)region(16), c->stream);
            ones.resize(m);
            if (e == hipSuccess) e = hipMemcpyAsync(ones.data(), region(16), m * 8, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return hip_fail(c, e, "ct_recrypt_exec (density)");
            for (uint64_t k = 0; k < m; ++k) {
                const long double total = (long double)cur[3][k] * (long double)m_bits;
                const double d = (double)((long double)ones[k] / total);
                (d < 0.495 || d > 0.505 ? cont : fin).push_back((uint32_t)k);
            }
        } else {
            fin = all;
        }
        if (!fin.empty()) {   // compact_edges + compact_layers into C's slots (recrypt.hpp:38-39)
            const uint64_t f = fin.size();
            view_up(fin, 0);
            std::vector<uint64_t> co(f);
            std::vector<uint32_t> fid(f);
            for (uint64_t k = 0; k < f; ++k) {
                fid[k] = cur_id[fin[k]];
                co[k] = hc[fid[k]];
                if (iters) iters[fid[k]] = (uint32_t)it;
            }
            if (e == hipSuccess) e = upload_words(c, region(12), co.data(), f * 8);
            for (uint64_t k = 0; k < f; ++k) co[k] = hc[n + fid[k]];
            if (e == hipSuccess) e = upload_words(c, region(14), co.data(), f * 8);
            if (e == hipSuccess) e = upload_words(c, c->recrypt.ids.get(), fid.data(), f * 4);
            if (e != hipSuccess) return hip_fail(c, e, "ct_recrypt_exec (compact views)");
            const pvac_ct_batch Xs = view_of(base, f, 0);
            pvac_ct_batch Cs = view_of(*C, f, 12);
            pvac_hip_plan cp;
            int rc = compact_classify(c, &Xs, &Cs, false, &cp);
            if (!rc) rc = compact_execute(c, &cp, &Xs, &Cs);
            if (rc) return rc;
            e = launch_scatter_counts(region(13), region(15), c->recrypt.ids.get(), f, C->l_cnt, C->e_cnt, c->stream);
            if (e != hipSuccess) return hip_fail(c, e, "ct_recrypt_exec (counts)");
        }
        if (cont.empty()) break;
        // ct_add of the picked pool members (recrypt.hpp:32-33), then ubk_apply (:34); ct_add has
        // applied guard_budget to the same edges, so :35 changes nothing
        const uint64_t m2 = cont.size();
        view_up(cont, 0);
        for (int f = 0; f < 4 && e == hipSuccess; ++f) {
            up.resize(m2);
            for (uint64_t k = 0; k < m2; ++k) up[k] = hp[f * pn + picks[8ull * cur_id[cont[k]] + it] % pn];
            e = upload_words(c, region(4 + f), up.data(), m2 * 8);
        }
        if (e != hipSuccess) return hip_fail(c, e, "ct_recrypt_exec (add views)");
        const pvac_ct_batch Av = view_of(base, m2, 0), Bv = view_of(*pool, m2, 4);
        pvac_ct_batch Cv{};
        Cv = view_of(Cv, m2, 8);
        Cv.sigma_words = sw;
        pvac_hip_plan ap;
        int rc = pvac_hip_ct_add_plan(c, &Av, &Bv, &Cv, &ap);
        if (rc) return rc;
        auto& buf = c->recrypt.buf[it & 1];
        const size_t nl = std::max<uint64_t>(ap.total_layer_slots, 1), ne = std::max<uint64_t>(ap.total_edge_slots, 1);
        e = buf.layers.grow(nl, nl);
        if (e == hipSuccess) e = buf.meta.grow(ne, ne);
        if (e == hipSuccess) e = buf.w_lo.grow(ne, ne);
        if (e == hipSuccess) e = buf.w_hi.grow(ne, ne);
        if (e == hipSuccess) e = buf.sigma.grow(ne * sw, ne * sw);
        if (e != hipSuccess) return hip_fail(c, e, "ct_recrypt_exec (alloc)");
        Cv.layers = buf.layers.get();
        Cv.meta = buf.meta.get();
        Cv.w_lo = buf.w_lo.get();
        Cv.w_hi = buf.w_hi.get();
        Cv.sigma = buf.sigma.get();
        rc = ct_add_exec(c, &ap, &Av, &Bv, 0, &Cv, deep_layer_bound(c->layer_limit));
        if (rc) return rc;
        for (uint64_t k = 0; k < m2; ++k)   // the sums above k_ct_add's table (the call then ran k_ct_add_deep)
            c->deep_route[3] += cur[1][cont[k]] + hp[pn + picks[8ull * cur_id[cont[k]] + it] % pn] > kAddLdsLayers;
        e = launch_ubk_apply(Cv, c->recrypt.ubk_perm.get(), m_bits, nullptr, c->num_cus, c->stream);
        // the next view: the sums, where ct_add put them
        std::vector<uint32_t> next_id(m2);
        for (uint64_t k = 0; k < m2; ++k) next_id[k] = cur_id[cont[k]];
        for (int f = 0; f < 4; ++f) {
            cur[f].assign(m2, 0);
            down(cur[f].data(), region(8 + f), m2);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "ct_recrypt_exec (step)");
        cur_id.swap(next_id);
        base = Cv;
    }
    return PVAC_OK;
} catch (...) { return caught(c, "ct_recrypt_exec"); }

}  // extern "C"
