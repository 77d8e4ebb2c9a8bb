// rt_ctx.cpp — libpvac_hip.so's host side, part 1 of the extern "C" ABI of include/pvac_hip.h: a
// context's life (create / destroy), its stream, timing, the last error, and the parameters set on
// it. The runtime is split by operation (rt_*.cpp) around the context of ctx.hpp: it owns the
// per-context device state (stream, libstdc++ bucket-count table, plan scratch, sparse H, timing
// events) and sequences the kernels. No unit throws across the ABI (ctx.hpp, caught()).
#include "ctx.hpp"

using namespace pvhip;

namespace {

void flush_timers(pvac_hip_ctx* c) {
    for (auto& kv : c->timing.timers) {
        for (auto& ev : kv.second.pending) {
            hipEventSynchronize(ev.second);
            float ms = 0;
            hipEventElapsedTime(&ms, ev.first, ev.second);
            kv.second.ms += ms;
            kv.second.launches += 1;
            c->timing.ev_pool.push_back(ev.first);
            c->timing.ev_pool.push_back(ev.second);
        }
        kv.second.pending.clear();
    }
}

// what pvac_hip_ctx_create puts into a new context; on failure the caller destroys it
int ctx_init(pvac_hip_ctx* c, int device, const pvac_hip_params* prm) {
    c->device = device;
    c->prm = *prm;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return PVAC_EDEVICE;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        c->num_cus = cus;
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return PVAC_EDEVICE;
    c->own_stream = true;
    std::vector<uint32_t> nb(kNbTableLen);
    std::vector<uint64_t> mg(kNbTableLen);
    for (uint32_t n = 0; n < kNbTableLen; ++n) {
        nb[n] = (uint32_t)bucket_count_after_reserve(n);
        mg[n] = make_fastmod64(nb[n]).m;
        if (nb[n] == 0 || nb[n] > 0xFFFFu) return PVAC_ERANGE;   // fresh_rec.nbk is u16
    }
    e = c->nb_table.grow(nb.size(), nb.size());
    if (e == hipSuccess) e = hipMemcpy(c->nb_table.get(), nb.data(), nb.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = c->nb_magic.grow(mg.size(), mg.size());
    if (e == hipSuccess) e = hipMemcpy(c->nb_magic.get(), mg.data(), mg.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = c->ps.init();
    if (e == hipSuccess) e = hipHostMalloc(&c->pin, 256, hipHostMallocDefault);
    return e == hipSuccess ? PVAC_OK : PVAC_ENOMEM;
}

}  // namespace

extern "C" {

int pvac_hip_abi_version(void) { return PVAC_HIP_ABI_VERSION; }

int pvac_hip_ctx_create(int device, const pvac_hip_params* prm, pvac_hip_ctx** out) {
    if (!out || !prm) return PVAC_EINVAL;
    *out = nullptr;
    if (prm->B == 0 || prm->B > 65535 || prm->m_bits == 0 || prm->n_bits == 0) return PVAC_EINVAL;
    pvac_hip_ctx* c = nullptr;
    const int rc = guarded(nullptr, "ctx_create", [&] {
        c = new pvac_hip_ctx();
        return ctx_init(c, device, prm);
    });
    if (rc) pvac_hip_ctx_destroy(c);
    else *out = c;
    return rc;
}

// The only deleter of a context (ctx_create's failure exit included): workers first, then this
// context's device, its stream drained, timer events, the stream-ordered buffers while the stream
// lives, the stream itself; the members' destructors free the rest before the caller's device returns.
int pvac_hip_ctx_destroy(pvac_hip_ctx* c) {
    if (!c) return PVAC_OK;
    for (pvac_hip_ctx* k : c->chain.kids) pvac_hip_ctx_destroy(k);
    device_guard dev(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (auto& kv : c->timing.timers)   // flush_timers returns events to the pool, which may allocate
        for (auto& ev : kv.second.pending) {
            hipEventDestroy(ev.first);
            hipEventDestroy(ev.second);
        }
    for (hipEvent_t e : c->timing.ev_pool) hipEventDestroy(e);
    c->worker.release(c->stream);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    if (c->pin) hipHostFree(c->pin);
    delete c;
    return PVAC_OK;
}

int pvac_hip_ctx_set_stream(pvac_hip_ctx* c, void* s) {
    if (!c) return PVAC_EINVAL;
    if (c->own_stream && c->stream) {
        hipStreamSynchronize(c->stream);
        hipStreamDestroy(c->stream);
        c->stream = nullptr;
        c->own_stream = false;
    }
    // NULL selects the legacy null stream (torch's default stream is 0): every launch and copy
    // is then ordered with the caller's own work on that stream.
    c->stream = (hipStream_t)s;
    c->own_stream = false;
    return PVAC_OK;
}

void* pvac_hip_ctx_stream(pvac_hip_ctx* c) { return c ? (void*)c->stream : nullptr; }

int pvac_hip_ctx_synchronize(pvac_hip_ctx* c) try {
    if (!c) return PVAC_EINVAL;
    return hip_fail(c, hipStreamSynchronize(c->stream), "synchronize");
} catch (...) { return caught(c, "synchronize"); }

int pvac_hip_ctx_set_noise(pvac_hip_ctx* c, double noise_entropy_bits, double tuple2_fraction, double depth_slope_bits) try {
    if (!c || !(noise_entropy_bits >= 0.0) || !(tuple2_fraction >= 0.0 && tuple2_fraction <= 1.0) ||
        !(depth_slope_bits >= 0.0) || noise_entropy_bits > 1e6 || depth_slope_bits > 1e6)
        return fail(c, PVAC_EINVAL, "ctx_set_noise: noise_entropy_bits, depth_slope_bits >= 0, tuple2_fraction in [0, 1]");
    c->prf.noise_bits = noise_entropy_bits;
    c->prf.noise_t2 = tuple2_fraction;
    c->prf.noise_slope = depth_slope_bits;
    return PVAC_OK;
} catch (...) { return caught(c, "ctx_set_noise"); }

int pvac_hip_ctx_set_powg(pvac_hip_ctx* c, const uint64_t* powg_host, uint32_t count) try {
    if (!c || !powg_host || count < c->prm.B) return fail(c, PVAC_EINVAL, "set_powg: need B (lo, hi) pairs");
    c->powg.release();
    c->powg_n = 0;
    hipError_t e = c->powg.grow(2 * (size_t)count, 2 * (size_t)count);
    if (e == hipSuccess) e = hipMemcpy(c->powg.get(), powg_host, (size_t)count * 16, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(c, e, "set_powg");
    c->powg_n = count;
    return PVAC_OK;
} catch (...) { return caught(c, "set_powg"); }

int pvac_hip_ctx_set_layer_limit(pvac_hip_ctx* c, uint32_t max_layers) try {
    if (!c) return PVAC_EINVAL;
    if (max_layers < PVAC_LAYER_LIMIT_DEFAULT || max_layers > PVAC_LAYER_LIMIT_MAX)
        return fail(c, PVAC_EINVAL, "ctx_set_layer_limit: the limit lies in [" + std::to_string(PVAC_LAYER_LIMIT_DEFAULT) + ", " +
                                        std::to_string(PVAC_LAYER_LIMIT_MAX) + "]");
    c->layer_limit = max_layers;
    return PVAC_OK;
} catch (...) { return caught(c, "ctx_set_layer_limit"); }

int pvac_hip_ctx_layer_limit(pvac_hip_ctx* c, uint32_t* out) {
    if (!c || !out) return PVAC_EINVAL;
    *out = c->layer_limit;
    return PVAC_OK;
}

int pvac_hip_deep_path_count(pvac_hip_ctx* c, uint64_t out[2]) {
    if (!c || !out) return PVAC_EINVAL;
    out[0] = c->mul.deep_total;
    out[1] = c->merge.deep_calls;
    return PVAC_OK;
}

int pvac_hip_deep_route_count(pvac_hip_ctx* c, uint64_t out[4]) {
    if (!c || !out) return PVAC_EINVAL;
    for (int k = 0; k < 4; ++k) out[k] = c->deep_route[k];
    return PVAC_OK;
}

int pvac_hip_ctx_set_enc_plan_limit(pvac_hip_ctx* c, uint32_t max_pre_edges) try {
    if (!c) return PVAC_EINVAL;
    if (max_pre_edges < PVAC_ENC_PLAN_LIMIT_DEFAULT || max_pre_edges > PVAC_ENC_PLAN_LIMIT_MAX)
        return fail(c, PVAC_EINVAL, "ctx_set_enc_plan_limit: the limit lies in [" + std::to_string(PVAC_ENC_PLAN_LIMIT_DEFAULT) +
                                        ", " + std::to_string(PVAC_ENC_PLAN_LIMIT_MAX) + "]");
    c->prf.enc_plan_limit = max_pre_edges;
    return PVAC_OK;
} catch (...) { return caught(c, "ctx_set_enc_plan_limit"); }

int pvac_hip_ctx_enc_plan_limit(pvac_hip_ctx* c, uint32_t* out) {
    if (!c || !out) return PVAC_EINVAL;
    *out = c->prf.enc_plan_limit;
    return PVAC_OK;
}

int pvac_hip_ctx_set_enc_budget(pvac_hip_ctx* c, uint64_t pre_edges) {
    if (!c) return PVAC_EINVAL;
    if (!pre_edges) return fail(c, PVAC_EINVAL, "ctx_set_enc_budget: a sub-batch holds at least one pre-merge edge");
    c->prf.enc_budget = pre_edges;
    return PVAC_OK;
}

int pvac_hip_ctx_enc_budget(pvac_hip_ctx* c, uint64_t* out) {
    if (!c || !out) return PVAC_EINVAL;
    *out = c->prf.enc_budget;
    return PVAC_OK;
}

int pvac_hip_enc_path_count(pvac_hip_ctx* c, uint64_t out[4]) {
    if (!c || !out) return PVAC_EINVAL;
    for (int k = 0; k < 4; ++k) out[k] = c->prf.enc_path[k];
    return PVAC_OK;
}

const char* pvac_hip_last_error(pvac_hip_ctx* c) { return c ? c->err.c_str() : "null context"; }

int pvac_hip_timing_enable(pvac_hip_ctx* c, int on) try {
    if (!c) return PVAC_EINVAL;
    c->timing.on = on != 0;
    // events for the launches to come, created now rather than inside the timed launches
    while (c->timing.on && c->timing.ev_pool.size() < 256) {
        hipEvent_t e{};
        if (hipEventCreate(&e) != hipSuccess) break;
        c->timing.ev_pool.push_back(e);
    }
    return PVAC_OK;
} catch (...) { return caught(c, "timing_enable"); }

int pvac_hip_timing_get(pvac_hip_ctx* c, const char* name, double* ms, uint64_t* launches) try {
    if (!c || !name) return PVAC_EINVAL;
    flush_timers(c);
    auto it = c->timing.timers.find(name);
    if (ms) *ms = it == c->timing.timers.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == c->timing.timers.end() ? 0 : it->second.launches;
    return PVAC_OK;
} catch (...) { return caught(c, "timing_get"); }

int pvac_hip_timing_reset(pvac_hip_ctx* c) try {
    if (!c) return PVAC_EINVAL;
    flush_timers(c);
    c->timing.timers.clear();
    return PVAC_OK;
} catch (...) { return caught(c, "timing_reset"); }

}  // extern "C"
