// rt_add.cpp — ct_add / ct_sub plan and exec, ct_scale, and the over-budget merge set that ct_add
// and compact (rt_recrypt.cpp) share.
#include "ctx.hpp"

using namespace pvhip;


namespace pvhip {

int merge_gather(pvac_hip_ctx* c, uint64_t n, const std::function<hipError_t(uint64_t*)>& gather,
                 const std::function<bool(const uint64_t*, merge_pair_info&)>& decode, const char* where,
                 const char* limit_msg) {
    std::vector<uint64_t> info(8 * n);
    hipError_t e = gather(c->ps.large_info.get());
    if (e == hipSuccess) e = hipMemcpyAsync(info.data(), c->ps.large_info.get(), info.size() * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, where);
    for (uint64_t k = 0; k < n; ++k) {
        merge_pair_info m{};
        if (!decode(&info[8 * k], m)) {
            c->merge.set.clear();
            return fail(c, PVAC_ENOSYS, limit_msg);
        }
        c->merge.set.push_back(m);
    }
    std::sort(c->merge.set.begin(), c->merge.set.end(),
              [](const merge_pair_info& x, const merge_pair_info& y) { return x.pair < y.pair; });
    return PVAC_OK;
}

// guard_budget (encrypt.hpp:106-111): compact_edges + compact_layers per item of the merge set
int merge_execute(pvac_hip_ctx* c, const pvac_ct_batch& A, const pvac_ct_batch& B, pvac_ct_batch& C, int negate_b,
                  const char* where) {
    if (const hipError_t e = c->merge.counters.grow(2, 2)) return hip_fail(c, e, "alloc merge counters");
    for (const merge_pair_info& m : c->merge.set) {
        const size_t need = merge_scratch_bytes(m.nA + m.nB, m.L);
        if (const hipError_t e = c->merge.scratch.grow(need, need)) return hip_fail(c, e, "alloc merge scratch");
        const int rc = hip_fail(c,
                                launch_add_merge(A, B, C, m.pair, m, c->prm.B, negate_b, c->merge.scratch.get(),
                                                 c->merge.scratch.capacity(), c->merge.counters.get(), c->stream),
                                where);
        if (rc) return rc;
    }
    return PVAC_OK;
}

}  // namespace pvhip

extern "C" {

int pvac_hip_ct_add_plan(pvac_hip_ctx* c, const pvac_ct_batch* A, const pvac_ct_batch* B, pvac_ct_batch* C,
                         pvac_hip_plan* plan) try {
    if (!c || !plan || !batch_ok(A) || !batch_ok(B) || !C || !C->l_off || !C->e_off)
        return fail(c, PVAC_EINVAL, "ct_add_plan: bad arguments");
    if (A->n != B->n) return fail(c, PVAC_EINVAL, "ct_add_plan: |A| != |B|");
    std::memset(plan, 0, sizeof *plan);
    plan->kind = 2;
    plan->n_pairs = A->n;
    C->n = A->n;
    if (!A->n) return PVAC_OK;
    c->merge.set.clear();
    plan_stats st;
    int rc = plan_pass(c, A->n, C, true, "ct_add_plan", [&] {
        return launch_plan_add(*A, *B, *C, c->ps.stats.get(), c->ps.pair_class.get(), c->ps.large_ids.get(), c->prm.edge_budget,
                               c->stream);
    }, st);
    if (rc) return rc;
    plan_fill(plan, A->n, st);
    if (st.n_large) {   // guard_budget pairs: shapes and offsets for the per-pair merge launches
        rc = merge_gather(
            c, st.n_large,
            [&](uint64_t* out) { return launch_gather_merge(*A, *B, *C, c->ps.large_ids.get(), st.n_large, out, c->stream); },
            [&](const uint64_t* o, merge_pair_info& m) {
                m.pair = o[0];
                m.LA = (uint32_t)o[1];
                m.L = (uint32_t)(o[1] + o[2]);
                m.nA = o[3];
                m.nB = o[4];
                m.aeo = o[5];
                m.beo = o[6];
                m.ceo = o[7];
                return !(m.nA + m.nB >= (1ull << 31) || (uint64_t)m.L * c->prm.B * 2 >= 0xFFFFFFFFull);
            },
            "ct_add_plan (merge)", "ct_add_plan: over-budget pair beyond 2^31 edges or 2^32 keys");
        if (rc) return rc;
    }
    c->ps.commit(plan);   // stamped only once it has succeeded, as in ct_mul_plan
    return PVAC_OK;
} catch (...) { return caught(c, "ct_add_plan"); }

int pvac_hip_ct_add_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* A, const pvac_ct_batch* B,
                         int negate_b, pvac_ct_batch* C) try {
    return ct_add_exec(c, plan, A, B, negate_b, C, c ? std::max<uint32_t>(kAddLdsLayers, c->layer_limit) : kAddLdsLayers);
} catch (...) { return caught(c, "ct_add_exec"); }

}  // extern "C"

int pvhip::ct_add_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* A, const pvac_ct_batch* B,
                       int negate_b, pvac_ct_batch* C, uint32_t lmax) {
    if (!c || !plan || plan->kind != 2 || !batch_ok(A) || !batch_ok(B) || !batch_ok(C))
        return fail(c, PVAC_EINVAL, "ct_add_exec: bad arguments");
    if (A->n != plan->n_pairs || B->n != plan->n_pairs) return fail(c, PVAC_EINVAL, "ct_add_exec: plan mismatch");
    if (!A->n) return PVAC_OK;
    if (plan->max_layers > lmax)
        return fail(c, PVAC_ENOSYS, "ct_add_exec: > " + std::to_string(lmax) + " layers per cipher");
    // a plan without over-budget pairs reads none of the plan scratch and stays valid
    if (plan->n_large && (!c->ps.is_latest(plan) || plan->n_large != c->merge.set.size()))
        return fail(c, PVAC_EINVAL, "ct_add_exec: plan is not this context's latest plan");
    if (plan->max_layers > kAddLdsLayers) {
        // beyond k_ct_add's LDS table: the whole call on k_ct_add_deep, a slab word per planned layer slot
        int rc = hip_fail(c, c->merge.deep_slab.grow_floor(std::max<uint64_t>(plan->total_layer_slots, 1)), "alloc ct_add slab");
        if (rc) return rc;
        scoped_timer t(c, "ct_add_deep");
        rc = hip_fail(c,
                      launch_ct_add_deep(*A, *B, *C, negate_b, c->merge.deep_slab.get(),
                                         plan->n_large ? c->ps.pair_class.get() : nullptr, c->stream),
                      "ct_add_deep");
        if (rc) return rc;
        ++c->merge.deep_calls;
    } else {
        scoped_timer t(c, "ct_add");
        const int rc = hip_fail(c,
                                launch_ct_add(*A, *B, *C, negate_b, plan->max_layers,
                                              plan->n_large ? c->ps.pair_class.get() : nullptr, c->stream),
                                "ct_add");
        if (rc) return rc;
    }
    if (!plan->n_large) return PVAC_OK;
    scoped_timer t(c, "ct_add_merge");
    return merge_execute(c, *A, *B, *C, negate_b, "ct_add merge");
}

extern "C" {

int pvac_hip_ct_scale(pvac_hip_ctx* c, pvac_ct_batch* X, uint64_t s_lo, uint64_t s_hi) try {
    if (!c || !batch_ok(X)) return PVAC_EINVAL;
    scoped_timer t(c, "ct_scale");
    return hip_fail(c, launch_ct_scale(*X, s_lo, s_hi, c->stream), "ct_scale");
} catch (...) { return caught(c, "ct_scale"); }

}  // extern "C"
