// rt_chain.cpp — pvac_hip_ct_mul_chain: depth chains of ct_mul over chunks of a batch, run by worker
// contexts (own stream, own scratch) on one thread each, over one or several devices.
#include <atomic>
#include <mutex>
#include <thread>

#include "ctx.hpp"

using namespace pvhip;

namespace {

struct chain_range {
    uint64_t end = 0;               // last input (exclusive) of this device range
    std::atomic<uint64_t> next{0};  // next chunk's first input
};

struct chain_shared {
    const pvac_ct_batch* X = nullptr;
    const pvac_chain_opts* o = nullptr;
    uint64_t chunk = 0;
    int x_dev = 0;                  // the device X (and the digest / count outputs) live on
    chain_range* ranges = nullptr;
    std::atomic<int> stop{0};
    std::mutex mu;
    int rc = PVAC_OK;
    std::string err;
    // the first failure is the chain's; called from a handler too, so it lets nothing out
    void failed(int code, const std::string& msg) noexcept {
        std::lock_guard<std::mutex> g(mu);
        if (rc == PVAC_OK) {
            rc = code;
            try {
                err = msg;
            } catch (...) {
                err.clear();
            }
        }
        stop.store(1);
    }
};

// a HIP call of the chain's workers: a failure stops the chain with "ct_mul_chain: <where>: <error>"
bool chain_ok(chain_shared* sh, hipError_t e, const char* where) {
    if (e == hipSuccess) return true;
    sh->failed(e == hipErrorOutOfMemory ? PVAC_ENOMEM : PVAC_EDEVICE,
               std::string("ct_mul_chain: ") + where + ": " + hipGetErrorString(e));
    return false;
}

struct chain_wstats {
    uint64_t gsum_pairs = 0, gsum_failed = 0, chunks = 0;
};

pvac_ct_batch chain_view(const pvac_ct_batch& X, uint64_t c0, uint64_t k) {
    pvac_ct_batch v = X;
    v.n = k;
    v.l_off = X.l_off + c0;
    v.l_cnt = X.l_cnt + c0;
    v.e_off = X.e_off + c0;
    v.e_cnt = X.e_cnt + c0;
    v.sigma = nullptr;
    v.sigma_words = 0;
    return v;
}

// the inputs of one chunk copied into the worker's own buffers (compact CSR): counts by peer
// copy, offsets by an exclusive scan, rows by k_stage_rows (peer reads when X lives elsewhere)
bool stage_chunk(pvac_hip_ctx* k, chain_shared* sh, const pvac_ct_batch& src, pvac_ct_batch& out, chain_set& S) {
    const uint64_t kk = src.n;
    if (!chain_ok(sh, S.grow_index(kk, k->stream), "stage alloc")) return false;
    if (ensure_scan(k, kk)) {
        sh->failed(PVAC_ENOMEM, "ct_mul_chain: stage scratch: " + k->err);
        return false;
    }
    const int sd = sh->x_dev, dd = k->device;
    if (!chain_ok(sh, hipMemcpyPeerAsync(S.l_cnt.get(), dd, src.l_cnt, sd, kk * 8, k->stream), "stage counts") ||
        !chain_ok(sh, hipMemcpyPeerAsync(S.e_cnt.get(), dd, src.e_cnt, sd, kk * 8, k->stream), "stage counts") ||
        !chain_ok(sh, hipMemcpyAsync(S.l_off.get(), S.l_cnt.get(), kk * 8, hipMemcpyDeviceToDevice, k->stream), "stage offsets") ||
        !chain_ok(sh, hipMemcpyAsync(S.e_off.get(), S.e_cnt.get(), kk * 8, hipMemcpyDeviceToDevice, k->stream), "stage offsets") ||
        !chain_ok(sh, launch_exclusive_scan_u64(S.l_off.get(), kk, k->scan_scratch.get(), &k->ps.totals[0], k->stream), "stage scan") ||
        !chain_ok(sh, launch_exclusive_scan_u64(S.e_off.get(), kk, k->scan_scratch.get(), &k->ps.totals[1], k->stream), "stage scan"))
        return false;
    unsigned long long tot[2] = {0, 0};
    if (!chain_ok(sh, hipMemcpyAsync(tot, k->ps.totals, sizeof tot, hipMemcpyDeviceToHost, k->stream), "stage totals") ||
        !chain_ok(sh, hipStreamSynchronize(k->stream), "stage totals"))
        return false;
    if (!chain_ok(sh, S.layers.grow_headroom(tot[0], k->stream), "stage alloc layers")) return false;
    for (dev_stream_buf<uint64_t>* b : {&S.meta, &S.w_lo, &S.w_hi})
        if (!chain_ok(sh, b->grow_headroom(tot[1], k->stream), "stage alloc edges")) return false;
    out = S.view(kk);
    return chain_ok(sh, launch_stage_rows(src, out, k->stream), "stage rows");
}

// the final step's sigmas (PVAC_MUL_WITH_SIGMA): salts from salts_at (or splitmix), then sigma_from_H
// per edge over the finished hash-order output; a pair the exec put in the canonical order
// (guard_budget / ORDER_CANONICAL) makes the step run once more with the salts mapped (exec's salt
// positions), as pvac_hip_ct_mul_exec does for a batch; that run reads A, which may still hold images
// (a_img), and writes records
bool chain_final_sigma(pvac_hip_ctx* k, chain_shared* sh, uint32_t d, uint64_t c0, pvac_hip_plan& plan,
                       const pvac_ct_batch& A, uint32_t* a_img, const pvac_ct_batch& Xv, pvac_ct_batch& C, chain_set& S,
                       uint32_t mflags) {
    const pvac_chain_opts& o = *sh->o;
    const uint64_t slots = std::max<uint64_t>(plan.total_edge_slots, 1);
    const uint32_t sw = k->prm.m_bits / 64;
    if (!chain_ok(sh, S.sigma.grow(slots * sw, slots * sw, k->stream), "sigma alloc (1 KiB per edge: a smaller chunk?)")) return false;
    if (!chain_ok(sh, k->worker.salts.grow_headroom(slots, k->stream), "sigma alloc salts")) return false;
    if (o.salts_at) {
        if (o.salts_at(o.user, d, c0, &A, &Xv, &C, k->worker.salts.get(), plan.total_edge_slots, (void*)k->stream) != 0) {
            sh->failed(PVAC_EINVAL, "ct_mul_chain: salts_at callback failed");
            return false;
        }
    } else if (o.flags & PVAC_CHAIN_DRBG) {
        if (drbg_fill(k, k->worker.salts.get(), (size_t)slots, "sigma fill salts")) {
            sh->failed(PVAC_EDEVICE, "ct_mul_chain: " + k->err);
            return false;
        }
    } else if (!chain_ok(sh,
                         launch_fill_random(o.nonce_seed ^ 0x5A175A175A175A17ull ^ (97ull * c0 + d), k->worker.salts.get(), slots,
                                            k->stream),
                         "sigma fill salts")) {
        return false;
    }
    C.sigma = S.sigma.get();
    C.sigma_words = sw;
    bool hash_order = (mflags & PVAC_MUL_ORDER_CANONICAL) == 0;
    if (hash_order) {
        std::vector<uint32_t> stv(C.n);
        if (!chain_ok(sh, hipMemcpyAsync(stv.data(), k->ps.pair_status.get(), C.n * 4, hipMemcpyDeviceToHost, k->stream), "sigma status") ||
            !chain_ok(sh, hipStreamSynchronize(k->stream), "sigma status"))
            return false;
        for (uint32_t v : stv) hash_order &= v != 1u;
    }
    if (hash_order) return chain_ok(sh, launch_sigma(k->H, k->prm, C, k->worker.salts.get(), nullptr, k->num_cus, k->stream), "sigma launch");
    if (ct_mul_exec(k, &plan, &A, &Xv, k->worker.nonces.get(), k->worker.salts.get(), &C, mflags | PVAC_MUL_WITH_SIGMA,
                    {a_img, nullptr, nullptr})) {
        sh->failed(PVAC_EDEVICE, "ct_mul_chain: sigma exec: " + k->err);
        return false;
    }
    return true;
}

// one worker: chunks of its device range in input order from the range's counter, depth steps of
// plan + exec each on this context's stream, the final c_depth to the digests / on_chunk
void chain_work(pvac_hip_ctx* k, chain_shared* sh, chain_range* rg, bool stage, chain_wstats* ws) {
    if (hipSetDevice(k->device) != hipSuccess) {
        sh->failed(PVAC_EDEVICE, "ct_mul_chain: hipSetDevice");
        return;
    }
    const pvac_chain_opts& o = *sh->o;
    const pvac_ct_batch& X = *sh->X;
    const uint32_t mflags = o.flags & PVAC_MUL_ORDER_CANONICAL;
    const bool check = (o.flags & PVAC_CHAIN_CHECK_GSUM) != 0;
    const bool sigma = (o.flags & PVAC_MUL_WITH_SIGMA) != 0;
    const bool remote = k->device != sh->x_dev;
    // intermediate steps hand their C to the next step as dense images (mul_large_args::C_img) unless
    // a caller hook or the gsum check reads every step's records; an image A never meets the fresh
    // kernel, whose pairs have at most kFreshEdgesMax < 2B edges a side
    const bool use_img = !check && !o.after_step && 2u * k->prm.B > kFreshEdgesMax;
    auto rcchk = [&](int rc, const char* where) {
        if (rc == PVAC_OK) return true;
        sh->failed(rc, std::string("ct_mul_chain: ") + where + ": " + k->err);
        return false;
    };
    for (;;) {
        if (sh->stop.load()) return;
        const uint64_t c0 = rg->next.fetch_add(sh->chunk);
        if (c0 >= rg->end) return;
        const uint64_t kk = std::min<uint64_t>(sh->chunk, rg->end - c0);
        pvac_ct_batch Xv = chain_view(X, c0, kk);
        if ((stage || remote) && !stage_chunk(k, sh, chain_view(X, c0, kk), Xv, k->worker.stage)) return;
        const pvac_ct_batch X0 = Xv;   // the chunk's inputs: c_0, and the operand of steps without one
        pvac_ct_batch A = Xv;
        int cur = 0;
        uint32_t* a_img = nullptr;   // the previous step's image flags (A's)
        for (uint32_t d = 0; d < o.depth; ++d) {
            if (sh->stop.load()) return;
            // this step's operand: operands[d] (the reference's loop multiplies by a fresh enc_value per
            // step, tests/test_main.cpp:291-292) or the chunk's inputs
            Xv = X0;
            if (d < o.n_operands) {
                Xv = chain_view(o.operands[d], c0, kk);
                if ((stage || remote) && !stage_chunk(k, sh, chain_view(o.operands[d], c0, kk), Xv, k->worker.stage_op))
                    return;
            }
            chain_set& S = k->worker.bufs[cur];
            if (!chain_ok(sh, S.grow_index(kk, k->stream), "alloc offsets / counts")) return;
            pvac_ct_batch C = S.view(kk);   // the plan writes its offsets and counts; the rows are sized below
            pvac_hip_plan plan{};
            if (!rcchk(pvac_hip_ct_mul_plan(k, &A, &Xv, &C, &plan), "plan")) return;
            // an output array that does not fit first takes this worker's scratch arena back (the
            // general path reallocates it within what is left, splitting its sub-batch if needed)
            auto grow_out = [&](auto& b, size_t need, const char* what) -> bool {
                hipError_t e = b.grow_headroom(need, k->stream);
                if (e == hipErrorOutOfMemory && k->mul.arena.get()) {
                    (void)hipGetLastError();
                    e = hipStreamSynchronize(k->stream);
                    k->mul.arena.release();
                    if (e == hipSuccess) e = b.grow_headroom(need, k->stream);
                }
                return chain_ok(sh, e, what);
            };
            if (!grow_out(S.layers, plan.total_layer_slots, "alloc layers") ||
                !grow_out(S.meta, plan.total_edge_slots, "alloc edges") ||
                !grow_out(S.w_lo, plan.total_edge_slots, "alloc edges") ||
                !grow_out(S.w_hi, plan.total_edge_slots, "alloc edges"))
                return;
            const size_t nw = 2 * std::max<uint64_t>(plan.total_layer_slots, 1);
            if (!chain_ok(sh, k->worker.nonces.grow_headroom(nw, k->stream), "alloc nonces")) return;
            C = S.view(kk);
            if (o.nonces_at) {
                if (o.nonces_at(o.user, d, c0, &A, &Xv, &C, k->worker.nonces.get(), nw, (void*)k->stream) != 0) {
                    sh->failed(PVAC_EINVAL, "ct_mul_chain: nonces_at callback failed");
                    return;
                }
            } else if (o.fill_nonces) {
                if (o.fill_nonces(o.user, d, c0, nw, k->worker.nonces.get(), (void*)k->stream) != 0) {
                    sh->failed(PVAC_EINVAL, "ct_mul_chain: fill_nonces callback failed");
                    return;
                }
            } else if (o.flags & PVAC_CHAIN_DRBG) {
                if (!rcchk(drbg_fill(k, k->worker.nonces.get(), nw, "fill nonces"), "generator")) return;
            } else if (!chain_ok(sh, launch_fill_random(o.nonce_seed + 97ull * c0 + d, k->worker.nonces.get(), nw, k->stream),
                               "fill nonces")) {
                return;
            }
            uint32_t* c_img = nullptr;
            if (use_img && d + 1 < o.depth) {
                if (!chain_ok(sh, S.img.grow_headroom(kk, k->stream), "alloc image flags")) return;
                if (!chain_ok(sh, hipMemsetAsync(S.img.get(), 0, kk * 4, k->stream), "image flags")) return;
                c_img = S.img.get();
            }
            const step_images img{a_img, c_img, k->worker.stats.get() + 2 * PVAC_CHAIN_MAX_DEPTH};
            if (!rcchk(ct_mul_exec(k, &plan, &A, &Xv, k->worker.nonces.get(), nullptr, &C, mflags, img), "exec")) return;
            if (!chain_ok(sh, launch_chain_stats(A, Xv, C, k->worker.stats.get() + 2 * d, k->stream), "stats")) return;
            if (check) {
                uint64_t bad = 0;
                if (!rcchk(pvac_hip_check_mul_gsum(k, &A, &Xv, &C, k->worker.nonces.get(), nullptr, &bad), "gsum check"))
                    return;
                ws->gsum_pairs += kk;
                ws->gsum_failed += bad;
            }
            if (o.after_step && o.after_step(o.user, d, c0, &A, &Xv, &C, nullptr, 0, (void*)k->stream) != 0) {
                sh->failed(PVAC_EINVAL, "ct_mul_chain: after_step callback failed");
                return;
            }
            if (sigma && d + 1 == o.depth && !chain_final_sigma(k, sh, d, c0, plan, A, a_img, Xv, C, S, mflags)) return;
            a_img = c_img;
            A = C;
            cur ^= 1;
        }
        // digests / counts land in the caller's arrays on X's device (through the worker's own
        // buffer and a peer copy when this worker runs on another device)
        auto out_words = [&](uint64_t n_out, uint64_t* dst, int kind) {   // 0 counts, 1 FNV, 2 sum digests
            if (n_out <= c0 || !dst) return true;
            const uint64_t m = std::min<uint64_t>(kk, n_out - c0);
            pvac_ct_batch H = A;
            H.n = m;
            auto put = [&](uint64_t* to) {
                if (kind == 1) return chain_ok(sh, launch_batch_digest(H, to, k->stream), "digest");
                if (kind == 2) return chain_ok(sh, launch_batch_sumdigest(H, to, k->stream), "sum digest");
                return chain_ok(sh, hipMemcpyAsync(to, A.e_cnt, m * 8, hipMemcpyDeviceToDevice, k->stream), "counts");
            };
            if (!remote) return put(dst + c0);
            if (!chain_ok(sh, k->worker.out.grow_headroom(m, k->stream), "alloc outputs") || !put(k->worker.out.get()))
                return false;
            return chain_ok(sh, hipMemcpyPeerAsync(dst + c0, sh->x_dev, k->worker.out.get(), k->device, m * 8, k->stream), "peer copy");
        };
        if (!out_words(o.digest_n, o.digest_out, 1) || !out_words(o.count_n, o.count_out, 0) ||
            !out_words(o.sumdigest_n, o.sumdigest_out, 2))
            return;
        if (o.on_chunk && o.on_chunk(o.user, c0, &A, (void*)k->stream) != 0) {
            sh->failed(PVAC_EINVAL, "ct_mul_chain: on_chunk callback failed");
            return;
        }
        ++ws->chunks;
    }
}

// a worker's thread: an exception that left it would end the process, so it stops the chain instead
void chain_worker(pvac_hip_ctx* k, chain_shared* sh, chain_range* rg, bool stage, chain_wstats* ws) noexcept {
    const int rc = guarded(k, "ct_mul_chain", [&] {
        chain_work(k, sh, rg, stage, ws);
        return PVAC_OK;
    });
    if (rc) sh->failed(rc, k->err);
}

// everything a chain worker grew during a call (its stream-ordered buffers, image scratch, the
// general-path arena, the gsum check's slabs); the caller selected the worker's device
hipError_t release_chain_worker(pvac_hip_ctx* k) {
    k->worker.release(k->stream);
    const hipError_t e = hipStreamSynchronize(k->stream);
    k->mul.img_tmp.release();
    k->mul.img_pairs.release();
    k->mul.arena.release();
    k->check.scratch.release();
    return e;
}

}  // namespace

extern "C" {

int pvac_hip_chain_partition(uint64_t n, uint64_t chunk, uint32_t parts, uint64_t* first) {
    if (!first || parts == 0 || parts > PVAC_CHAIN_MAX_DEVICES) return PVAC_EINVAL;
    if (!chunk) chunk = 1024;
    const uint64_t nch = (n + chunk - 1) / chunk;   // whole chunks, dealt as evenly as possible
    for (uint32_t j = 0; j <= parts; ++j) first[j] = std::min<uint64_t>(n, (nch * j / parts) * chunk);
    return PVAC_OK;
}

int pvac_hip_ct_mul_chain(pvac_hip_ctx* c, const pvac_ct_batch* X, const pvac_chain_opts* o, pvac_chain_stats* st) try {
    if (!c || !o || !st || !batch_ok(X)) return fail(c, PVAC_EINVAL, "ct_mul_chain: bad arguments");
    if (o->depth < 1 || o->depth > PVAC_CHAIN_MAX_DEPTH) return fail(c, PVAC_EINVAL, "ct_mul_chain: depth");
    if (o->flags & ~(PVAC_MUL_ORDER_CANONICAL | PVAC_CHAIN_CHECK_GSUM | PVAC_MUL_WITH_SIGMA | PVAC_CHAIN_STAGE_INPUTS |
                     PVAC_CHAIN_IMG_BATCH2 | PVAC_CHAIN_DRBG))
        return fail(c, PVAC_EINVAL, "ct_mul_chain: flags");
    if (o->n_operands > o->depth || (o->n_operands && !o->operands))
        return fail(c, PVAC_EINVAL, "ct_mul_chain: operands");
    for (uint32_t d = 0; d < o->n_operands; ++d) {
        const pvac_ct_batch& Y = o->operands[d];
        if (!batch_ok(&Y) || Y.n != X->n || (Y.n && (!Y.layers || !Y.meta || !Y.w_lo || !Y.w_hi)))
            return fail(c, PVAC_EINVAL, "ct_mul_chain: operand " + std::to_string(d) + " is not a batch of |X| ciphers");
    }
    if ((o->flags & PVAC_CHAIN_CHECK_GSUM) && !c->powg.get())
        return fail(c, PVAC_EINVAL, "ct_mul_chain: CHECK_GSUM needs pvac_hip_ctx_set_powg");
    if ((o->flags & PVAC_MUL_WITH_SIGMA) && !c->H.ready)
        return fail(c, PVAC_EINVAL, "ct_mul_chain: WITH_SIGMA needs H (pvac_hip_ctx_set_H / gen_H)");
    if (o->n_devices > PVAC_CHAIN_MAX_DEVICES || (o->n_devices && !o->devices))
        return fail(c, PVAC_EINVAL, "ct_mul_chain: devices");
    if (X->n && (!X->layers || !X->meta || !X->w_lo || !X->w_hi)) return fail(c, PVAC_EINVAL, "ct_mul_chain: input arrays");
    std::memset(st, 0, sizeof *st);
    const auto t0 = std::chrono::steady_clock::now();
    if (!X->n) return PVAC_OK;
    const uint32_t S = o->streams ? std::min<uint32_t>(o->streams, 64) : 4u;
    const uint64_t chunk = o->chunk ? o->chunk : 1024;
    const uint32_t D = o->n_devices ? o->n_devices : 1u;
    std::vector<int> devs(D, c->device);
    for (uint32_t j = 0; j < o->n_devices; ++j) devs[j] = o->devices[j];
    // inputs already enqueued on the caller's stream must be complete before other streams read them
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "ct_mul_chain (caller stream)");
    // a layout change (streams, chunk, the device list) first returns everything the workers grew
    // (output batches, nonce / salt / result words, image scratch, scratch arenas), so the HBM shares
    // below are taken over the device's memory, not over what the previous layout's workers left free
    std::vector<int64_t> layout{(int64_t)S, (int64_t)chunk, (int64_t)D};
    layout.insert(layout.end(), devs.begin(), devs.end());
    device_guard dev(c->device);   // the loops below select the workers' devices
    if (!c->chain.kids.empty() && layout != c->chain.layout) {
        for (pvac_hip_ctx* k : c->chain.kids) {
            hipSetDevice(k->device);
            e = release_chain_worker(k);
            if (e != hipSuccess) return hip_fail(c, e, "ct_mul_chain: worker release");
        }
    }
    c->chain.layout = layout;
    // worker contexts: [range j * S + w] on devs[j]; a layout change rebuilds the ones that differ
    if (c->chain.kids.size() > (size_t)D * S) {
        for (size_t w = (size_t)D * S; w < c->chain.kids.size(); ++w) pvac_hip_ctx_destroy(c->chain.kids[w]);
        c->chain.kids.resize((size_t)D * S);
    }
    for (uint32_t j = 0; j < D; ++j) {
        // each worker's general-path scratch: its share of half the HBM free now on its device (the
        // other half holds the workers' ping-pong outputs and the caller's data)
        size_t free_b = 0, total_b = 0;
        if (hipSetDevice(devs[j]) != hipSuccess)
            return fail(c, PVAC_EDEVICE, "ct_mul_chain: device " + std::to_string(devs[j]));
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 8ull << 30;
        const uint32_t same = (uint32_t)std::count(devs.begin(), devs.end(), devs[j]);
        const uint64_t cap_words = std::max<uint64_t>((uint64_t)(free_b / 2) / ((uint64_t)S * same) / 4, 1ull << 24);
        if (devs[j] != c->device) {   // peer reads of X / peer writes of the outputs
            const hipError_t pe = hipDeviceEnablePeerAccess(c->device, 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled)
                return hip_fail(c, pe, "ct_mul_chain: peer access");
            (void)hipGetLastError();
        }
        for (uint32_t w = 0; w < S; ++w) {
            const size_t slot = (size_t)j * S + w;
            if (slot < c->chain.kids.size() && c->chain.kids[slot]->device != devs[j]) {
                pvac_hip_ctx_destroy(c->chain.kids[slot]);
                c->chain.kids[slot] = nullptr;
            }
            if (slot >= c->chain.kids.size()) c->chain.kids.push_back(nullptr);
            pvac_hip_ctx*& k = c->chain.kids[slot];
            if (!k) {
                const int rc = pvac_hip_ctx_create(devs[j], &c->prm, &k);
                if (rc) return fail(c, rc, "ct_mul_chain: worker context");
            }
            e = k->worker.stats.grow(2 * PVAC_CHAIN_MAX_DEPTH + 1, 2 * PVAC_CHAIN_MAX_DEPTH + 1);
            if (e != hipSuccess) return hip_fail(c, e, "ct_mul_chain: worker statistics");
            k->worker.arena_cap_words = cap_words;
            k->prm = c->prm;
            k->layer_limit = c->layer_limit;
            k->worker.spin_us = 200;
            k->worker.img_grid_y = (o->flags & PVAC_CHAIN_IMG_BATCH2) ? 2u : 65535u;
            if (c->powg.get() && (k->powg_n != c->powg_n || !k->powg.get())) {
                k->powg.release();
                e = k->powg.grow(2 * (size_t)c->powg_n, 2 * (size_t)c->powg_n);
                if (e != hipSuccess) return hip_fail(c, e, "ct_mul_chain: worker powg");
                k->powg_n = c->powg_n;
            }
            // the worker's generator: 48 bytes of the caller's, drawn when the worker is created (and
            // again after the caller's generator was seeded anew, so an explicit seed reaches it)
            if ((o->flags & PVAC_CHAIN_DRBG) && k->drbg.worker_from != c->drbg.epoch) {
                uint8_t seed[kDrbgSeedLen];
                int rc = c->drbg.gen.generate_host(seed, sizeof seed);
                uint64_t cnt[4];
                c->drbg.gen.counts(cnt);
                if (!rc) rc = k->drbg.gen.seed(seed, cnt[3] != 0);
                wipe(seed, sizeof seed);
                if (rc) return fail(c, rc, "ct_mul_chain: worker generator: no entropy (getrandom failed)");
                k->drbg.worker_from = c->drbg.epoch;
            }
            e = hipSuccess;
            if (c->powg.get()) e = hipMemcpyPeer(k->powg.get(), k->device, c->powg.get(), c->device, (size_t)c->powg_n * 16);
            if (e == hipSuccess && (o->flags & PVAC_MUL_WITH_SIGMA) && (!k->H.ready || k->worker.H_from != c->H_gen)) {
                e = sigma_tables_clone(k->H, c->H, k->device, c->device, k->stream);
                k->worker.H_from = c->H_gen;
            }
            if (e == hipSuccess) e = hipMemsetAsync(k->worker.stats.get(), 0, (2 * PVAC_CHAIN_MAX_DEPTH + 1) * 8, k->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(k->stream);
            if (e != hipSuccess) return hip_fail(c, e, "ct_mul_chain: worker setup");
        }
    }
    std::vector<uint64_t> first(D + 1);
    pvac_hip_chain_partition(X->n, chunk, D, first.data());
    std::vector<chain_range> ranges(D);
    for (uint32_t j = 0; j < D; ++j) {
        ranges[j].next.store(first[j]);
        ranges[j].end = first[j + 1];
    }
    chain_shared sh;
    sh.X = X;
    sh.o = o;
    sh.chunk = chunk;
    sh.x_dev = c->device;
    sh.ranges = ranges.data();
    const size_t nk = (size_t)D * S;
    std::vector<chain_wstats> ws(nk);
    std::vector<uint64_t> redo0(nk);
    std::vector<uint64_t> deep0(nk);
    for (size_t w = 0; w < nk; ++w) {
        redo0[w] = c->chain.kids[w]->mul.redo_total;
        deep0[w] = c->chain.kids[w]->mul.deep_total;
    }
    std::vector<std::thread> th;
    th.reserve(nk);
    try {
        for (uint32_t j = 0; j < D; ++j)
            for (uint32_t w = 0; w < S; ++w)
                th.emplace_back(chain_worker, c->chain.kids[(size_t)j * S + w], &sh, &ranges[j],
                                j > 0 && (o->flags & PVAC_CHAIN_STAGE_INPUTS) != 0, &ws[(size_t)j * S + w]);
    } catch (...) {   // a thread that could not start: none may stay joinable when th goes
        sh.stop.store(1);
        for (std::thread& t : th) t.join();
        throw;
    }
    for (std::thread& t : th) t.join();
    for (size_t w = 0; w < nk; ++w) {
        pvac_hip_ctx* k = c->chain.kids[w];
        hipSetDevice(k->device);
        e = hipStreamSynchronize(k->stream);
        if (e != hipSuccess && sh.rc == PVAC_OK) {
            hip_fail(c, e, "ct_mul_chain");
            sh.failed(PVAC_EDEVICE, c->err);
        }
        unsigned long long v[2 * PVAC_CHAIN_MAX_DEPTH + 1];
        if (hipMemcpy(v, k->worker.stats.get(), sizeof v, hipMemcpyDeviceToHost) == hipSuccess) {
            for (uint32_t d = 0; d < o->depth; ++d) {
                st->edges[d] += v[2 * d];
                st->products[d] += v[2 * d + 1];
            }
            st->image_steps += v[2 * PVAC_CHAIN_MAX_DEPTH];
        }
        st->gsum_pairs += ws[w].gsum_pairs;
        st->gsum_failed += ws[w].gsum_failed;
        st->chunks += ws[w].chunks;
        st->redo += k->mul.redo_total - redo0[w];
        c->mul.deep_total += k->mul.deep_total - deep0[w];   // pvac_hip_deep_path_count counts the workers' pairs
    }
    st->pair_steps = X->n * o->depth;
    st->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (sh.rc != PVAC_OK) return fail(c, sh.rc, sh.err);
    return PVAC_OK;
} catch (...) { return caught(c, "ct_mul_chain"); }

}  // extern "C"
