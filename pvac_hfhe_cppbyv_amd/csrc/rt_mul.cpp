// rt_mul.cpp — ct_mul: plan, exec (the fresh kernel, the general path, the redo run), its status and
// its path counters.
#include <cstdio>
#include <cstdlib>

#include "ctx.hpp"

using namespace pvhip;

namespace {

// Pairs whose bucket count is at least twice their key-slot space (dense chain steps: reserve(|A.E||B.E|)
// buckets for |A.L||B.L|B slots) share their bucket groups with every pair of the same bucket count:
// the group of a slot depends only on (slot, B, bucket count). One static table per distinct bucket
// count replaces the per-pair bucket table + chains (k_large_link) and its zeroing; rank walks the
// static group and keeps the slots present in the pair (almost every slot is alone in its bucket).
// Builds the tables of `set` into the context's one buffer (c->mul.grp: they replace those of any other
// set) and rebuilds the descriptors of its pairs that use them; allow_direct = false keeps every
// pair on the full layout (per-key sums: the redo run, the canonical order).
int assign_static_groups(pvac_hip_ctx* c, std::vector<large_desc>& set, bool allow_direct) {
    constexpr size_t kMaxCfg = 64;
    constexpr uint64_t kMaxWords = 1ull << 28;   // <= 1 GiB of tables
    std::map<uint64_t, uint64_t> cfg;             // bucket count -> max S
    for (const large_desc& d : set)
        if (d.nbm.d >= 2 * d.S && d.S && !is_deep(d)) {   // a deep pair keeps its dynamic chains
            uint64_t& m = cfg[d.nbm.d];
            m = std::max(m, d.S);
        }
    uint64_t words = 0, tmp_max = 0;
    for (auto& kv : cfg) {
        words += 2 * kv.second;
        tmp_max = std::max<uint64_t>(tmp_max, 1ull << std::max<uint32_t>(1, ceil_log2(2 * kv.second)));
    }
    if (cfg.empty() || cfg.size() > kMaxCfg || words > kMaxWords) return PVAC_OK;   // dynamic chains
    int rc = hip_fail(c, c->mul.grp.grow_floor(words), "alloc bucket-group tables");
    if (!rc) rc = hip_fail(c, c->mul.grp_tmp.grow_floor(3 * tmp_max), "alloc bucket-group scratch");
    if (rc) return rc;
    std::map<uint64_t, uint64_t> off;   // bucket count -> head offset (next = head + S_max)
    uint64_t o = 0;
    for (auto& kv : cfg) {
        const uint64_t Sm = kv.second;
        const uint32_t hb = std::max<uint32_t>(1, ceil_log2(2 * Sm));
        const uint64_t hcap = 1ull << hb;
        unsigned long long* tk = (unsigned long long*)c->mul.grp_tmp.get();   // [hcap] u64 keys, then [hcap] u32 heads
        uint32_t* th = c->mul.grp_tmp.get() + 2 * hcap;
        hipError_t e = hipMemsetAsync(c->mul.grp_tmp.get(), 0, 3 * hcap * 4, c->stream);
        if (e == hipSuccess)
            e = launch_grp_build(make_fastmod64(kv.first), c->prm.B, Sm, hb, c->mul.grp.get() + o, c->mul.grp.get() + o + Sm, tk, th,
                                 c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "build bucket-group tables");
        off[kv.first] = o;
        o += 2 * Sm;
    }
    for (large_desc& d : set) {
        auto it = off.find(d.nbm.d);
        if (it == off.end() || d.nbm.d < 2 * d.S || !d.S || is_deep(d)) continue;
        std::string why;
        large_desc x;
        rc = build_large_desc(x, d.pair, d.LA, d.LB, d.nA, d.nB, c->prm.B, why, true,
                              allow_direct && c->prm.edge_budget < (1ull << 28) &&   // 8-byte offsets < 2^31
                                  !slots_share_bucket(d.nbm.d, d.S, c->prm.B));
        if (rc) return fail(c, rc, why);
        x.g_head = it->second;
        x.g_next = it->second + cfg[d.nbm.d];
        d = x;
    }
    return PVAC_OK;
}

// Shapes of the pairs ids[0, n) read back -> host descriptors on the dynamic layout (bucket counts
// from this libstdc++), in pair order: a deterministic launch order (the kernels append ids in
// arrival order). `out` is left empty on failure.
int gather_large_descs(pvac_hip_ctx* c, const pvac_ct_batch* A, const pvac_ct_batch* B, const uint64_t* ids, uint64_t n,
                       std::vector<large_desc>& out, const char* where) {
    out.clear();
    std::vector<uint64_t> info(5 * n);
    hipError_t e = launch_gather_large(*A, *B, ids, n, c->ps.large_info.get(), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(info.data(), c->ps.large_info.get(), info.size() * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, where);
    out.resize(n);
    for (uint64_t k = 0; k < n; ++k) {
        std::string why;
        const int rc = build_large_desc(out[k], info[5 * k], info[5 * k + 1], info[5 * k + 2], info[5 * k + 3],
                                        info[5 * k + 4], c->prm.B, why, false, false, c->layer_limit);
        if (rc) {
            out.clear();
            return fail(c, rc, why);
        }
    }
    std::sort(out.begin(), out.end(), [](const large_desc& x, const large_desc& y) { return x.pair < y.pair; });
    return PVAC_OK;
}

}  // namespace

extern "C" int pvac_hip_ct_mul_plan(pvac_hip_ctx* c, const pvac_ct_batch* A, const pvac_ct_batch* B, pvac_ct_batch* C,
                                    pvac_hip_plan* plan) try {
    if (!c || !plan || !batch_ok(A) || !batch_ok(B) || !C || !C->l_off || !C->e_off)
        return fail(c, PVAC_EINVAL, "ct_mul_plan: bad arguments");
    if (A->n != B->n) return fail(c, PVAC_EINVAL, "ct_mul_plan: |A| != |B|");
    std::memset(plan, 0, sizeof *plan);
    plan->kind = 1;
    plan->n_pairs = A->n;
    C->n = A->n;
    c->mul.set.clear();
    // every earlier plan goes stale now; this one is stamped valid only once it has succeeded, so
    // exec rejects a plan whose device work or descriptor build failed
    if (!A->n) {
        c->ps.invalidate();
        c->ps.commit(plan);
        return PVAC_OK;
    }
    plan_stats st;
    int rc = plan_pass(c, A->n, C, true, "ct_mul_plan", [&] {
        return launch_plan_mul(*A, *B, *C, c->ps.pair_class.get(), c->ps.large_ids.get(), c->ps.stats.get(), c->nb_table.get(),
                               kNbTableLen, c->prm.B, c->stream);
    }, st);
    if (rc) return rc;
    plan_fill(plan, A->n, st);
    if (st.n_large) {
        rc = gather_large_descs(c, A, B, c->ps.large_ids.get(), st.n_large, c->mul.set, "ct_mul_plan (large)");
        if (!rc) rc = assign_static_groups(c, c->mul.set, true);
        if (rc) {
            c->mul.set.clear();
            return rc;
        }
    }
    c->ps.commit(plan);
    return PVAC_OK;
} catch (...) { return caught(c, "ct_mul_plan"); }

namespace {

// A chain step's input held as dense images (img.in) turned back into hash-order records for the
// pairs given as (pair, |A.E|) before a path that reads A's records (the non-direct kernels, the
// redo run). The device skips pairs whose flag is clear and clears the flags of the pairs it converts.
int images_to_records(pvac_hip_ctx* c, const pvac_ct_batch* A, const std::vector<std::pair<uint64_t, uint64_t>>& pn,
                      step_images img) {
    if (!img.in || pn.empty()) return PVAC_OK;
    std::vector<uint64_t> h(2 * pn.size());
    uint64_t tot = 0;
    for (size_t k = 0; k < pn.size(); ++k) {
        h[k] = pn[k].first;
        h[pn.size() + k] = tot;
        tot += pn[k].second;
    }
    int rc = hip_fail(c, c->mul.img_pairs.grow_floor(h.size()), "alloc image pairs");
    if (!rc) rc = hip_fail(c, c->mul.img_tmp.grow_floor(3 * std::max<uint64_t>(tot, 1)), "alloc image scratch");
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(c->mul.img_pairs.get(), h.data(), h.size() * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = launch_image_to_records(*A, img.in, c->mul.img_pairs.get(), (uint32_t)pn.size(), c->mul.img_tmp.get(), c->prm.B,
                                    c->worker.img_grid_y, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // h is read from the host stack
    return e == hipSuccess ? PVAC_OK : hip_fail(c, e, "chain images to records");
}

// Runs the general path over `set` (pair order, static groups assigned) in sub-batches that fit the
// scratch budget (cut_sub_batch, large_plan.hpp).
int run_large(pvac_hip_ctx* c, const std::vector<large_desc>& set, const pvac_ct_batch* A, const pvac_ct_batch* B,
              const uint64_t* nonces, pvac_ct_batch* C, uint32_t flags, uint32_t* salt_pos, step_images img) {
    const size_t nl = set.size();
    int rc = hip_fail(c, c->mul.desc_dev.grow_floor(nl), "alloc large descriptors");
    if (!rc) rc = hip_fail(c, c->mul.sel_dev.grow_floor(nl), "alloc large descriptor order");
    if (rc) return rc;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 8ull << 30;
    uint64_t budget = std::max<uint64_t>((uint64_t)(free_b / 2) / 4 + c->mul.arena.capacity(), 1ull << 24);
    budget = std::min<uint64_t>(budget, 16ull << 30);   // <= 64 GiB of scratch per sub-batch
    // a worker of pvac_hip_ct_mul_chain shares the device with the other workers: its share
    if (c->worker.arena_cap_words) budget = std::min<uint64_t>(budget, std::max<uint64_t>(c->worker.arena_cap_words, c->mul.arena.capacity()));
    sub_batch& sb = c->mul.sub;
    size_t i = 0;
    while (i < nl) {
        // the uploads below read sb's vectors when the stream reaches them: the previous sub-batch's
        // must have been taken before its storage is cut anew
        if (i && hipStreamSynchronize(c->stream) != hipSuccess) return hip_fail(c, hipErrorUnknown, "ct_mul_large");
        cut_sub_batch(set, i, budget, sb);
        if (sb.words > c->mul.arena.capacity()) {
            // grow with 1/8 headroom (within the budget): batches of similar pairs differ by a few
            // words, and a free + re-malloc of tens of GB stalls for seconds
            uint64_t grown = std::max<uint64_t>(sb.words, std::min<uint64_t>(sb.words + sb.words / 8, budget));
            hipStreamSynchronize(c->stream);
            const auto t0 = std::chrono::steady_clock::now();
            hipError_t e = c->mul.arena.grow(sb.words, grown);   // frees the old arena first
            if (e == hipErrorOutOfMemory && grown > sb.words) {   // without the headroom
                (void)hipGetLastError();
                grown = sb.words;
                e = c->mul.arena.grow(sb.words, grown);
            }
            if (e == hipErrorOutOfMemory && sb.end - i > 1) {
                // other contexts hold the HBM the budget counted on: split this sub-batch and retry
                (void)hipGetLastError();
                budget = std::max<uint64_t>(sb.words / 2, 1);
                continue;
            }
            if (e != hipSuccess) return hip_fail(c, e, "alloc ct_mul scratch arena");
            if (std::getenv("PVAC_DEBUG_ARENA"))
                std::fprintf(stderr, "[pvac] arena -> %.2f GB (free %.1f GB, sub-batch %zu pairs): %.1f ms\n",
                             grown * 4e-9, free_b * 1e-9, sb.end - i,
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        hipError_t e = hipMemcpyAsync(c->mul.desc_dev.get() + i, sb.desc.data(), sb.desc.size() * sizeof(large_desc),
                                      hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(c->mul.sel_dev.get() + i, sb.sel.data(), sb.sel.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                               c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "upload large descriptors");
        mul_large_args a = sb.sizing;
        a.A = *A; a.B = *B; a.C = *C;
        a.nonces = nonces;
        a.pair_status = c->ps.pair_status.get();
        a.desc = c->mul.desc_dev.get() + i;
        a.scratch = c->mul.arena.get();
        a.Bm = c->prm.B;
        a.canon_tag = c->prm.canon_tag;
        a.edge_budget = c->prm.edge_budget;
        a.flags = flags;
        a.salt_pos = salt_pos;
        a.grp = c->mul.grp.get();
        a.sel = c->mul.sel_dev.get() + i;
        a.redo_ids = c->ps.redo_ids.get();
        a.redo_cnt = c->ps.redo_cnt.get();
        a.A_img = img.in;
        a.C_img = img.out;
        a.img_count = img.out ? img.count : nullptr;
        if (a.deep) {
            // its own lists and layers kernels around the shared stages, each under its timing name
            for (int stage = 0; stage < kDeepStages && e == hipSuccess; ++stage) {
                if (stage == 1 || stage == 3) {
                    scoped_timer t(c, stage == 1 ? "large_lists_deep" : "large_layers_deep");
                    e = launch_ct_mul_large_deep(a, stage, c->stream);
                } else {
                    e = launch_ct_mul_large_deep(a, stage, c->stream);
                }
            }
            if (e == hipSuccess) c->mul.deep_total += sb.end - i;
        } else {
            e = launch_ct_mul_large(a, c->stream);
        }
        if (e != hipSuccess) return hip_fail(c, e, "ct_mul_large");
        c->mul.path_total[1] += sb.end - i;
        c->mul.path_total[2] += sb.n_iblk;
        c->mul.path_total[3] += sb.n_direct;
        i = sb.end;
    }
    return PVAC_OK;
}

// The fresh kernel and the general path's direct mode emit every key cell that received a
// product; a cell whose sum is 0 mod p (cancelling products or a zero weight, arithmetic.hpp:98-99)
// makes them flag the pair instead, and a direct pair that needs the canonical order or shares
// buckets is flagged too. Those pairs are re-run here on the general path's full layout, which
// folds every sum before it orders keys.
int redo_fresh_pairs(pvac_hip_ctx* c, const pvac_ct_batch* A, const pvac_ct_batch* B, const uint64_t* nonces,
                     pvac_ct_batch* C, uint32_t flags, uint32_t* salt_pos, step_images img) {
    unsigned int cnt = 0;
    hipError_t e = read_back(c, &cnt, c->ps.redo_cnt.get(), sizeof cnt);
    if (e != hipSuccess) return hip_fail(c, e, "ct_mul_exec (redo count)");
    if (!cnt) {
        c->ps.redo_cnt_dirty = false;
        return PVAC_OK;
    }
    std::vector<large_desc> redo;
    int rc = gather_large_descs(c, A, B, c->ps.redo_ids.get(), cnt, redo, "ct_mul_exec (redo shapes)");
    if (rc) return rc;
    // a chain step's image inputs become records first; the redo run reads and writes records only
    if (img.in) {
        std::vector<std::pair<uint64_t, uint64_t>> pn;
        for (const large_desc& d : redo) pn.emplace_back(d.pair, d.nA);
        rc = images_to_records(c, A, pn, img);
        if (rc) return rc;
    }
    // the exact path: per-key sums, no presence-based positions. The group tables become the redo
    // set's, so the plan's own are rebuilt afterwards
    rc = assign_static_groups(c, redo, false);
    if (!rc) rc = run_large(c, redo, A, B, nonces, C, flags, salt_pos, {});
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = hip_fail(c, hipErrorUnknown, "ct_mul_exec (redo)");
    if (!rc) {
        c->mul.redo_total += cnt;
        if (!c->mul.set.empty()) rc = assign_static_groups(c, c->mul.set, true);
    }
    // on failure the group tables may still belong to the redo set: no exec may reuse this plan
    if (rc) c->ps.invalidate();
    return rc;
}

}  // namespace

int pvhip::ct_mul_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* A, const pvac_ct_batch* B,
                const uint64_t* nonces, const uint64_t* salts, pvac_ct_batch* C, uint32_t flags, step_images img) {
    if (!c || !plan || plan->kind != 1 || !batch_ok(A) || !batch_ok(B) || !batch_ok(C))
        return fail(c, PVAC_EINVAL, "ct_mul_exec: bad arguments");
    if (A->n != plan->n_pairs || B->n != plan->n_pairs) return fail(c, PVAC_EINVAL, "ct_mul_exec: plan mismatch");
    if (!A->n) return PVAC_OK;
    if (!c->ps.is_latest(plan) || plan->n_large != c->mul.set.size())
        return fail(c, PVAC_EINVAL, "ct_mul_exec: plan is not this context's latest ct_mul plan");
    if (!nonces) return fail(c, PVAC_EINVAL, "ct_mul_exec: nonces required");
    if (!C->layers || !C->meta || !C->w_lo || !C->w_hi) return fail(c, PVAC_EINVAL, "ct_mul_exec: output arrays");
    c->mul.last_pairs = 0;   // pair_status is valid again only once this exec has launched its kernels
    const bool with_sigma = (flags & PVAC_MUL_WITH_SIGMA) != 0;
    if (with_sigma && (!salts || !C->sigma || !c->H.ready))
        return fail(c, PVAC_EINVAL, "ct_mul_exec: WITH_SIGMA needs salts, C->sigma and H");
    uint32_t* salt_pos = nullptr;
    if (with_sigma) {
        int rc = hip_fail(c, c->mul.salt_pos.grow_floor(plan->total_edge_slots), "alloc salt positions");
        if (rc) return rc;
        salt_pos = c->mul.salt_pos.get();
    }
    if (c->ps.redo_cnt_dirty) {   // a read-back of zero leaves it clean: no memset per exec
        const hipError_t e = hipMemsetAsync(c->ps.redo_cnt.get(), 0, sizeof(unsigned int), c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "reset redo count");
    }
    c->ps.redo_cnt_dirty = true;   // until this exec reads back a zero count
    c->mul.path_total[0] += plan->n_small;
    if (plan->n_small) {
        mul_fresh_args a;
        std::memset(&a, 0, sizeof a);   // padding too: the upload below is skipped on equal bytes
        a.A = *A; a.B = *B; a.C = *C;
        a.recs = c->ps.fresh_recs.get();
        a.nonces = nonces;
        a.pair_class = c->ps.pair_class.get();
        a.pair_status = c->ps.pair_status.get();
        a.nb_table = c->nb_table.get();
        a.nb_magic = c->nb_magic.get();
        a.salt_pos = salt_pos;
        a.redo_ids = c->ps.redo_ids.get();
        a.redo_cnt = c->ps.redo_cnt.get();
        a.canon_tag = c->prm.canon_tag;
        a.edge_budget = c->prm.edge_budget;
        a.Bm = c->prm.B;
        a.flags = flags;
        a.ks_max = std::max<uint32_t>(plan->max_keys, 32u);   // LDS sizing floor (0-key batches)
        a.prod_max = plan->max_prod;
        a.na_max = plan->max_na;
        a.nb_max = plan->max_nb;
        a.buckets_max = plan->max_buckets;
        a.layers_max = plan->max_layers;
        {
            scoped_timer t(c, "mul_layers_fresh");
            hipError_t e = launch_mul_layers_fresh(a, c->stream);
            if (e != hipSuccess) return hip_fail(c, e, "mul_layers_fresh");
        }
        if (const hipError_t ea = c->mul.fresh_args.grow(1, 1)) return hip_fail(c, ea, "alloc fresh args");
        // stream-ordered copy from the ctx's host mirror (kept alive until the next exec); a batch
        // exec'd again into the same buffers (the kernels never write their arguments) reuses it
        hipError_t e = hipSuccess;
        if (!c->mul.fresh_args_uploaded || std::memcmp(&c->mul.fresh_args_host, &a, sizeof a) != 0) {
            c->mul.fresh_args_uploaded = false;
            std::memcpy(&c->mul.fresh_args_host, &a, sizeof a);
            e = hipMemcpyAsync(c->mul.fresh_args.get(), &c->mul.fresh_args_host, sizeof a, hipMemcpyHostToDevice, c->stream);
            c->mul.fresh_args_uploaded = e == hipSuccess;
        }
        if (e != hipSuccess) return hip_fail(c, e, "upload fresh args");
        scoped_timer t(c, "ct_mul_fresh");
        e = launch_ct_mul_fresh(a, c->mul.fresh_args.get(), c->num_cus, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "ct_mul_fresh");
    }
    if (plan->n_large && (flags & PVAC_MUL_ORDER_CANONICAL) &&
        std::any_of(c->mul.set.begin(), c->mul.set.end(), [](const large_desc& d) { return d.direct != 0; })) {
        // the direct mode emits hash order only: with the canonical order asked for, its pairs would
        // all be redone, so take them on the full layout from the start (descriptors rebuilt once;
        // the plan stays valid, its direct pairs now run the exact path)
        const int rc = assign_static_groups(c, c->mul.set, false);
        if (rc) {
            c->ps.invalidate();
            return rc;
        }
    }
    if (plan->n_large && img.in) {   // chain step: image inputs of pairs off the direct mode -> records
        std::vector<std::pair<uint64_t, uint64_t>> pn;
        for (const large_desc& d : c->mul.set)
            if (!d.direct) pn.emplace_back(d.pair, d.nA);
        const int rc = images_to_records(c, A, pn, img);
        if (rc) return rc;
    }
    if (plan->n_large) {
        scoped_timer t(c, "ct_mul_large");
        int rc = run_large(c, c->mul.set, A, B, nonces, C, flags, salt_pos, img);
        if (rc) return rc;
    }
    {
        int rc = redo_fresh_pairs(c, A, B, nonces, C, flags, salt_pos, img);
        if (rc) return rc;
    }
    c->mul.last_pairs = A->n;
    if (with_sigma) {
        scoped_timer t(c, "sigma");
        hipError_t e = launch_sigma(c->H, c->prm, *C, salts, salt_pos, c->num_cus, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "sigma");
    }
    return PVAC_OK;
}

extern "C" {

int pvac_hip_ct_mul_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* A, const pvac_ct_batch* B,
                         const uint64_t* nonces, const uint64_t* salts, pvac_ct_batch* C, uint32_t flags) try {
    return ct_mul_exec(c, plan, A, B, nonces, salts, C, flags, {});
} catch (...) { return caught(c, "ct_mul_exec"); }

int pvac_hip_ct_mul(pvac_hip_ctx* c, const pvac_ct_batch* A, const pvac_ct_batch* B, pvac_ct_batch* C,
                    uint64_t layer_cap, uint64_t edge_cap, const uint64_t* nonces, const uint64_t* salts,
                    uint32_t flags, pvac_hip_plan* plan_out) try {
    pvac_hip_plan p{};
    int rc = pvac_hip_ct_mul_plan(c, A, B, C, &p);
    if (plan_out) *plan_out = p;
    if (rc) return rc;
    if (p.total_layer_slots > layer_cap || p.total_edge_slots > edge_cap) {
        c->ps.invalidate();   // the plan's offsets do not fit C: it is not exec'd
        return fail(c, PVAC_ENOMEM, "ct_mul: output capacity below the plan's totals");
    }
    return pvac_hip_ct_mul_exec(c, &p, A, B, nonces, salts, C, flags);
} catch (...) { return caught(c, "ct_mul"); }

int pvac_hip_ct_mul_redo_count(pvac_hip_ctx* c, uint64_t* out) {
    if (!c || !out) return PVAC_EINVAL;
    *out = c->mul.redo_total;
    return PVAC_OK;
}

int pvac_hip_ct_mul_path_count(pvac_hip_ctx* c, uint64_t* out) {
    if (!c || !out) return PVAC_EINVAL;
    for (int k = 0; k < 4; ++k) out[k] = c->mul.path_total[k];
    return PVAC_OK;
}

int pvac_hip_ct_mul_status(pvac_hip_ctx* c, uint32_t* out, size_t n) try {
    if (!c || (!out && n)) return fail(c, PVAC_EINVAL, "ct_mul_status: bad arguments");
    if (!n) return PVAC_OK;
    if (n > c->mul.last_pairs) return fail(c, PVAC_EINVAL, "ct_mul_status: more pairs than the last ct_mul_exec held");
    const hipError_t e = hipMemcpyAsync(out, c->ps.pair_status.get(), n * 4, hipMemcpyDeviceToDevice, c->stream);
    return e == hipSuccess ? PVAC_OK : hip_fail(c, e, "ct_mul_status");
} catch (...) { return caught(c, "ct_mul_status"); }

}  // extern "C"
