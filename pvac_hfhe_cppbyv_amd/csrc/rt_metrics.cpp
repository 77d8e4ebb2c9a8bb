// rt_metrics.cpp — the per-cipher metrics of utils/metrics.hpp: sigma byte histograms (sigma_shannon's
// counts) and per-layer gsums (agg_layer_gsum), with the counters of the routes they took.
#include "ctx.hpp"

using namespace pvhip;

extern "C" {

int pvac_hip_sigma_bytehist(pvac_hip_ctx* c, const pvac_ct_batch* X, uint64_t* hist) try {
    if (!c || !batch_ok(X) || (!hist && X->n)) return fail(c, PVAC_EINVAL, "sigma_bytehist: bad arguments");
    if (!X->n) return PVAC_OK;
    if (!sigma_ok(c, X)) return fail(c, PVAC_EINVAL, "sigma_bytehist: X carries no sigma of m_bits");
    if (X->n > 0x7FFFFFFFull) return fail(c, PVAC_ENOSYS, "sigma_bytehist: more than 2^31 - 1 ciphers");
    int wide = 0;
    scoped_timer t(c, "sigma_bytehist");
    const int rc = hip_fail(c, launch_sigma_bytehist(*X, c->prm.m_bits, c->num_cus, (unsigned long long*)hist, &wide, c->stream),
                            "sigma_bytehist");
    if (!rc) c->metrics.path[wide ? 0 : 1]++;
    return rc;
} catch (...) { return caught(c, "sigma_bytehist"); }

int pvac_hip_layer_gsum(pvac_hip_ctx* c, const pvac_ct_batch* X, uint64_t* gsum, uint32_t* status) try {
    if (!c || !batch_ok(X)) return fail(c, PVAC_EINVAL, "layer_gsum: bad arguments");
    if (!c->powg.get()) return fail(c, PVAC_EINVAL, "layer_gsum: powg_B not set (pvac_hip_ctx_set_powg)");
    if (!X->n) return PVAC_OK;
    if (!gsum || !X->meta || !X->w_lo || !X->w_hi) return fail(c, PVAC_EINVAL, "layer_gsum: null arrays");
    // the size pass: the largest layer tables (LDS size, slabs) and the route counts, one read-back
    hipError_t e = c->metrics.sizes.grow(kGsumSizeWords + 1, kGsumSizeWords + 1);
    unsigned long long* dev = c->metrics.sizes.get();
    if (e == hipSuccess) e = hipMemsetAsync(dev, 0, kGsumSizeWords * 8, c->stream);
    if (e == hipSuccess) e = launch_gsum_sizes(*X, dev, c->stream);
    unsigned long long sz[kGsumSizeWords] = {};
    if (e == hipSuccess) e = read_back(c, sz, dev, sizeof sz);
    if (e != hipSuccess) return hip_fail(c, e, "layer_gsum (sizes)");
    if (sz[6]) return fail(c, PVAC_ENOSYS, "layer_gsum: a cipher of 2^28 layers or more");
    const uint64_t sb = gsum_slab_bytes(X->n, sz, c->num_cus);
    if (sb) {
        const int rc = hip_fail(c, c->metrics.slabs.grow_floor((size_t)sb), "alloc layer_gsum slabs");
        if (rc) return rc;
    }
    scoped_timer t(c, "layer_gsum");
    const int rc = hip_fail(c,
                            launch_layer_gsum(*X, c->powg.get(), c->prm.B, sz, gsum, status, sb ? c->metrics.slabs.get() : nullptr,
                                              dev + kGsumSizeWords, c->num_cus, c->stream),
                            "layer_gsum");
    if (rc) return rc;
    for (int k = 0; k < 3; ++k) c->metrics.path[2 + k] += sz[2 + k];
    return PVAC_OK;
} catch (...) { return caught(c, "layer_gsum"); }

int pvac_hip_metrics_path_count(pvac_hip_ctx* c, uint64_t out[5]) {
    if (!c || !out) return PVAC_EINVAL;
    for (int k = 0; k < 5; ++k) out[k] = c->metrics.path[k];
    return PVAC_OK;
}

}  // extern "C"
