// rt_util.cpp — what stands beside the cipher operations: Fp arithmetic, the ALU probes, the gsum
// check of a ct_mul step, synthetic batches and nonces, digests, commit_ct, batch_pack, memcpy.
#include "commit_msg.hpp"
#include "ctx.hpp"

using namespace pvhip;

extern "C" {

// ---------------------------------------------------------------- Fp
int pvac_hip_fp_binop(pvac_hip_ctx* c, int op, const uint64_t* a_lo, const uint64_t* a_hi, const uint64_t* b_lo,
                      const uint64_t* b_hi, uint64_t* c_lo, uint64_t* c_hi, size_t n) try {
    if (!c) return PVAC_EINVAL;
    if (op < PVAC_FP_ADD || op > PVAC_FP_INV) return fail(c, PVAC_EINVAL, "fp_binop: bad op");
    if (n && (!a_lo || !a_hi || !c_lo || !c_hi)) return fail(c, PVAC_EINVAL, "fp_binop: null array");
    if (n && op != PVAC_FP_NEG && op != PVAC_FP_INV && (!b_lo || !b_hi)) return fail(c, PVAC_EINVAL, "fp_binop: null b");
    scoped_timer t(c, "fp_binop");
    return hip_fail(c, launch_fp_binop(op, a_lo, a_hi, b_lo, b_hi, c_lo, c_hi, n, c->stream), "fp_binop");
} catch (...) { return caught(c, "fp_binop"); }

// ---------------------------------------------------------------- measured ALU ceilings
int pvac_hip_alu_ceiling(pvac_hip_ctx* c, int kind, double* per_s) try {
    if (!c || !per_s || kind < 0 || kind > 5) return fail(c, PVAC_EINVAL, "alu_ceiling: bad arguments");
    const hipError_t e = run_alu_probe(kind, c->num_cus, c->stream, per_s);
    return e == hipSuccess ? PVAC_OK : hip_fail(c, e, "alu_ceiling");
} catch (...) { return caught(c, "alu_ceiling"); }

int pvac_hip_issue_probe(pvac_hip_ctx* c, int op, int waves_per_simd, double* per_s, double* clock_hz) try {
    if (!c || !per_s || !clock_hz) return fail(c, PVAC_EINVAL, "issue_probe: bad arguments");
    const hipError_t e = run_issue_probe(op, waves_per_simd, c->num_cus, c->stream, per_s, clock_hz);
    return e == hipSuccess ? PVAC_OK : hip_fail(c, e, "issue_probe");
} catch (...) { return caught(c, "issue_probe"); }

// ---------------------------------------------------------------- gsum invariant
int pvac_hip_check_mul_gsum(pvac_hip_ctx* c, const pvac_ct_batch* A, const pvac_ct_batch* B, const pvac_ct_batch* C,
                            const uint64_t* nonces, uint32_t* status, uint64_t* n_bad) try {
    if (!c || !n_bad || !batch_ok(A) || !batch_ok(B) || !batch_ok(C) || !nonces)
        return fail(c, PVAC_EINVAL, "check_mul_gsum: bad arguments");
    if (A->n != B->n || A->n != C->n) return fail(c, PVAC_EINVAL, "check_mul_gsum: batch sizes differ");
    if (!c->powg.get()) return fail(c, PVAC_EINVAL, "check_mul_gsum: powg_B not set (pvac_hip_ctx_set_powg)");
    *n_bad = 0;
    if (!A->n) return PVAC_OK;
    hipError_t e = c->check.buf.grow(8, 8);
    if (e == hipSuccess) e = hipMemsetAsync(c->check.buf.get(), 0, 32, c->stream);
    if (e == hipSuccess) e = launch_check_sizes(*A, *B, *C, c->check.buf.get(), c->stream);
    unsigned int mx[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(mx, c->check.buf.get(), sizeof mx, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "check_mul_gsum (sizes)");
    unsigned long long* cnt = (unsigned long long*)(c->check.buf.get() + 4);
    // layer tables beyond one workgroup's LDS (chain depth 9 on): per-workgroup slabs in global memory
    const uint64_t gs = check_gsum_scratch_bytes(c->prm.B, mx, A->n, c->num_cus);
    if (gs) {
        const int rc = hip_fail(c, c->check.scratch.grow_floor((size_t)gs), "alloc gsum check scratch");
        if (rc) return rc;
    }
    e = launch_check_gsum(*A, *B, *C, nonces, c->powg.get(), c->prm.B, mx, status, cnt, c->num_cus, gs ? c->check.scratch.get() : nullptr,
                          c->stream);
    if (e == hipErrorInvalidValue) return fail(c, PVAC_ERANGE, "check_mul_gsum: no scratch for the layer tables");
    unsigned long long bad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, cnt, sizeof bad, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "check_mul_gsum");
    c->check.path[gs ? 1 : 0]++;
    *n_bad = bad;
    return PVAC_OK;
} catch (...) { return caught(c, "check_mul_gsum"); }

int pvac_hip_check_mul_gsum_path_count(pvac_hip_ctx* c, uint64_t out[2]) {
    if (!c || !out) return PVAC_EINVAL;
    out[0] = c->check.path[0];
    out[1] = c->check.path[1];
    return PVAC_OK;
}

// ---------------------------------------------------------------- synthetic / checks
int pvac_hip_gen_fresh_batch(pvac_hip_ctx* c, uint64_t seed, uint32_t epl, pvac_ct_batch* X) {
    return pvac_hip_gen_fresh_batch_at(c, seed, 0, epl, X);
}

int pvac_hip_gen_fresh_batch_at(pvac_hip_ctx* c, uint64_t seed, uint64_t first_index, uint32_t epl,
                                pvac_ct_batch* X) try {
    if (!c || !batch_ok(X) || !X->layers || !X->meta || !X->w_lo || !X->w_hi) return PVAC_EINVAL;
    return hip_fail(c, launch_gen_fresh(seed, first_index, epl, c->prm.B, *X, c->stream), "gen_fresh");
} catch (...) { return caught(c, "gen_fresh_batch"); }

int pvac_hip_fill_nonces(pvac_hip_ctx* c, uint64_t seed, uint64_t first_index, const pvac_ct_batch* A,
                         const pvac_ct_batch* B, const pvac_ct_batch* C, uint64_t* out) try {
    if (!c || !batch_ok(A) || !batch_ok(B) || !C || !C->l_off || (A->n && !out) || A->n != B->n) return PVAC_EINVAL;
    return hip_fail(c, launch_fill_nonces(seed, first_index, *A, *B, C->l_off, out, c->stream), "fill_nonces");
} catch (...) { return caught(c, "fill_nonces"); }

int pvac_hip_fill_random(pvac_hip_ctx* c, uint64_t seed, uint64_t* out, size_t n) try {
    if (!c || (n && !out)) return PVAC_EINVAL;
    return hip_fail(c, launch_fill_random(seed, out, n, c->stream), "fill_random");
} catch (...) { return caught(c, "fill_random"); }

uint64_t pvac_hip_bucket_count(uint64_t n) { return bucket_count_after_reserve(n); }

int pvac_hip_batch_digest(pvac_hip_ctx* c, const pvac_ct_batch* X, uint64_t* out) try {
    if (!c || !batch_ok(X) || (X->n && !out)) return PVAC_EINVAL;
    return hip_fail(c, launch_batch_digest(*X, out, c->stream), "batch_digest");
} catch (...) { return caught(c, "batch_digest"); }

int pvac_hip_commit_ct(pvac_hip_ctx* c, const pvac_ct_batch* X, uint8_t* digests) try {
    if (!c || !batch_ok(X) || (X->n && !digests)) return fail(c, PVAC_EINVAL, "commit_ct: bad arguments");
    if (!c->have_digest) return fail(c, PVAC_EINVAL, "commit_ct: H_digest unknown (gen_H, set_H or set_H_digest)");
    if (X->sigma && (uint64_t)X->sigma_words * 64 < c->prm.m_bits)
        return fail(c, PVAC_EINVAL, "commit_ct: sigma rows of " + std::to_string(X->sigma_words) + " words are shorter than m_bits");
    if (!X->n) return PVAC_OK;
    if (!X->layers || !X->meta || !X->w_lo || !X->w_hi) return fail(c, PVAC_EINVAL, "commit_ct: null row arrays");
    if (const hipError_t e = c->commit_counter.grow(1, 1)) return hip_fail(c, e, "alloc commit counter");
    uint32_t head[kCommitHeadWords];
    commit_head_words(c->H_digest, c->prm.canon_tag, head);
    const uint32_t sigma_bytes = X->sigma ? (c->prm.m_bits + 7) / 8 : 0;
    scoped_timer t(c, "commit_ct");
    return hip_fail(c, launch_commit_ct(*X, head, sigma_bytes, c->num_cus, c->commit_counter.get(), digests, c->stream),
                    "commit_ct");
} catch (...) { return caught(c, "commit_ct"); }

int pvac_hip_batch_sumdigest(pvac_hip_ctx* c, const pvac_ct_batch* X, uint64_t* out) try {
    if (!c || !batch_ok(X) || (X->n && !out)) return PVAC_EINVAL;
    return hip_fail(c, launch_batch_sumdigest(*X, out, c->stream), "batch_sumdigest");
} catch (...) { return caught(c, "batch_sumdigest"); }

// The used rows of a capacity-padded batch packed back to back (a plan's output keeps every pair's
// capacity): dst's counts = src's, its offsets their exclusive scans, rows (and sigma when both
// carry it) copied by k_stage_rows. totals[0], [1] = the packed layer / edge counts, so a caller
// copies exactly those rows to the host. dst's row arrays must hold the packed rows (src's
// capacity always does); the pair scratch of a pending plan is left alone.
int pvac_hip_batch_pack(pvac_hip_ctx* c, const pvac_ct_batch* src, pvac_ct_batch* dst, uint64_t* totals) try {
    if (!c || !batch_ok(src) || !dst || !totals) return fail(c, PVAC_EINVAL, "batch_pack: arguments");
    const uint64_t n = src->n;
    if (n && (!dst->l_off || !dst->l_cnt || !dst->e_off || !dst->e_cnt || !dst->layers || !dst->meta || !dst->w_lo ||
              !dst->w_hi || !src->layers || !src->meta || !src->w_lo || !src->w_hi))
        return fail(c, PVAC_EINVAL, "batch_pack: null arrays");
    if (dst->sigma && (!src->sigma || dst->sigma_words != src->sigma_words))
        return fail(c, PVAC_EINVAL, "batch_pack: dst sigma needs src sigma of the same width");
    dst->n = n;
    totals[0] = totals[1] = 0;
    if (!n) return PVAC_OK;
    int rc = ensure_scan(c, n);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(dst->l_cnt, src->l_cnt, n * 8, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dst->e_cnt, src->e_cnt, n * 8, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dst->l_off, src->l_cnt, n * 8, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dst->e_off, src->e_cnt, n * 8, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess)
        e = launch_exclusive_scan2_u64(dst->l_off, dst->e_off, n, c->scan_scratch.get(), &c->ps.totals[0], &c->ps.totals[1],
                                       c->stream);
    unsigned long long tot[2] = {0, 0};
    if (e == hipSuccess) e = read_back(c, tot, c->ps.totals, sizeof tot);
    if (e != hipSuccess) return hip_fail(c, e, "batch_pack (offsets)");
    totals[0] = tot[0];
    totals[1] = tot[1];
    return hip_fail(c, launch_stage_rows(*src, *dst, c->stream), "batch_pack (rows)");
} catch (...) { return caught(c, "batch_pack"); }

int pvac_hip_memcpy(void* dst, const void* src, size_t bytes, void* stream) {
    if (!bytes) return PVAC_OK;
    if (!dst || !src) return PVAC_EINVAL;
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? PVAC_OK : PVAC_EDEVICE;
}

}  // extern "C"
