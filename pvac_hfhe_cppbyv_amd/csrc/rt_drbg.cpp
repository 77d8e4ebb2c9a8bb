// rt_drbg.cpp — the device CSPRNG of the ABI: the context's CTR_DRBG (drbg.hpp) with its keystream
// written by k_aes256_ctr (k_drbg.hip), and the raw keystream entry pvac_hip_aes256_ctr.
#include "ctx.hpp"

using namespace pvhip;

namespace pvhip {

// The host state advances inside request(), before the launch: two fills enqueued back to back,
// from one thread or two, never share a counter. The job's round keys are wiped once the launch has
// copied them into its kernel arguments.
int drbg_fill(pvac_hip_ctx* c, uint64_t* out, size_t n_words, const char* where) {
    if (!n_words) return PVAC_OK;
    aes_ctr_job job;
    int rc = c->drbg.gen.request(n_words, &job);
    if (rc) {
        wipe(&job, sizeof job);
        return fail(c, rc, std::string(where) + ": no entropy (getrandom failed)");
    }
    {
        scoped_timer t(c, "aes256_ctr");
        rc = hip_fail(c, launch_aes256_ctr(job, out, n_words, c->stream), where);
    }
    wipe(&job, sizeof job);
    return rc;
}

}  // namespace pvhip

extern "C" {

int pvac_hip_aes256_ctr(pvac_hip_ctx* c, const uint8_t key[32], const uint8_t ctr_be[16], uint64_t* out, size_t n_words) try {
    if (!c) return PVAC_EINVAL;
    if (!key || !ctr_be || (n_words && !out)) return fail(c, PVAC_EINVAL, "aes256_ctr: null argument");
    if (!n_words) return PVAC_OK;
    aes_ctr_job job;
    aes256_host_expand(key, job.rk);
    job.ctr_hi = job.ctr_lo = 0;
    for (int i = 0; i < 8; ++i) {
        job.ctr_hi = (job.ctr_hi << 8) | ctr_be[i];
        job.ctr_lo = (job.ctr_lo << 8) | ctr_be[8 + i];
    }
    job.nb = ((uint64_t)n_words + 1) / 2;
    int rc;
    {
        scoped_timer t(c, "aes256_ctr");
        rc = hip_fail(c, launch_aes256_ctr(job, out, n_words, c->stream), "aes256_ctr");
    }
    wipe(&job, sizeof job);
    return rc;
} catch (...) { return caught(c, "aes256_ctr"); }

int pvac_hip_drbg_seed(pvac_hip_ctx* c, const uint8_t seed[48]) try {
    if (!c) return PVAC_EINVAL;
    const int rc = c->drbg.gen.seed(seed);
    if (rc) return fail(c, rc, "drbg_seed: no entropy (getrandom failed)");
    ++c->drbg.epoch;
    return PVAC_OK;
} catch (...) { return caught(c, "drbg_seed"); }

int pvac_hip_drbg_reseed(pvac_hip_ctx* c, const uint8_t entropy[48]) try {
    if (!c) return PVAC_EINVAL;
    const int rc = c->drbg.gen.reseed(entropy);
    return rc ? fail(c, rc, "drbg_reseed: no entropy (getrandom failed)") : PVAC_OK;
} catch (...) { return caught(c, "drbg_reseed"); }

int pvac_hip_drbg_fill(pvac_hip_ctx* c, uint64_t* out, size_t n_words) try {
    if (!c) return PVAC_EINVAL;
    if (n_words && !out) return fail(c, PVAC_EINVAL, "drbg_fill: null out");
    return drbg_fill(c, out, n_words, "drbg_fill");
} catch (...) { return caught(c, "drbg_fill"); }

int pvac_hip_drbg_counts(pvac_hip_ctx* c, uint64_t out[4]) {
    if (!c || !out) return PVAC_EINVAL;
    c->drbg.gen.counts(out);
    return PVAC_OK;
}

int pvac_hip_drbg_tile(uint32_t out[2]) {
    if (!out) return PVAC_EINVAL;
    out[0] = kDrbgTile;
    out[1] = kDrbgGridCap;
    return PVAC_OK;
}

}  // extern "C"
