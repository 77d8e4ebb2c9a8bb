// runtime.cpp — host side of libpvac_hip.so: the extern "C" ABI of include/pvac_hip.h.
//
// Owns per-context device state (stream, libstdc++ bucket-count table, plan scratch,
// sparse H, timing events) and sequences the kernels. Never throws across the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <new>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "commit_msg.hpp"
#include "common.hpp"
#include "dev_mem.hpp"
#include "large_plan.hpp"
#include "sigma.hpp"
#include "sha256.hpp"

using namespace pvhip;

namespace {

constexpr uint32_t kNbTableLen = kFreshProdMax + 1;   // bucket counts for |A.E||B.E| in [0, 4096]

struct timer_rec {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double ms = 0;
    uint64_t launches = 0;
};

// one output batch of a chain worker (pvac_hip_ct_mul_chain): stream-ordered allocations that grow
struct chain_set {
    dev_stream_buf<uint64_t> l_off, l_cnt, e_off, e_cnt;
    dev_stream_buf<pvac_layer> layers;
    dev_stream_buf<uint64_t> meta, w_lo, w_hi;
    dev_stream_buf<uint64_t> sigma;   // final step with PVAC_MUL_WITH_SIGMA: 1 KiB per edge slot
    dev_stream_buf<uint32_t> img;     // per pair: 1 = this step's C is a dense image (mul_large_args::C_img)
    void release(hipStream_t st) {
        for (dev_stream_buf<uint64_t>* b : {&l_off, &l_cnt, &e_off, &e_cnt, &meta, &w_lo, &w_hi, &sigma}) b->release(st);
        layers.release(st);
        img.release(st);
    }
    // the four per-cipher arrays for n ciphers
    hipError_t grow_index(size_t n, hipStream_t st) {
        hipError_t e = hipSuccess;
        for (dev_stream_buf<uint64_t>* b : {&l_off, &l_cnt, &e_off, &e_cnt})
            if (e == hipSuccess) e = b->grow_headroom(n, st);
        return e;
    }
    // the batch of n ciphers over the buffers as they are now (no sigma)
    pvac_ct_batch view(uint64_t n) const {
        pvac_ct_batch v{};
        v.n = n;
        v.l_off = l_off.get();
        v.l_cnt = l_cnt.get();
        v.layers = layers.get();
        v.e_off = e_off.get();
        v.e_cnt = e_cnt.get();
        v.meta = meta.get();
        v.w_lo = w_lo.get();
        v.w_hi = w_hi.get();
        return v;
    }
};

}  // namespace

struct pvac_hip_ctx {
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    pvac_hip_params prm{};
    std::string err;
    // device tables / scratch
    dev_buf<uint32_t> nb_table;
    dev_buf<uint64_t> nb_magic;
    // the pair scratch, grown together by ensure_pairs (8 words of large_info per pair)
    dev_buf<uint8_t> pair_class;
    dev_buf<uint32_t> pair_status;
    dev_buf<fresh_rec> fresh_recs;   // per-pair header records of the fresh ct_mul path
    dev_buf<uint64_t> large_ids, large_info;
    dev_buf<uint64_t> redo_ids;      // fresh-kernel pairs left to the general path (a key sum of 0)
    dev_buf<unsigned int> redo_cnt;
    std::vector<merge_pair_info> merge_host;   // over-budget ct_add pairs of the latest add plan
    dev_buf<uint8_t> merge_scratch;
    dev_buf<unsigned long long> merge_counters;
    dev_buf<uint64_t> powg;            // pk.powg_B on the device, B x (lo, hi)
    uint32_t powg_n = 0;
    dev_buf<uint8_t> dec_scratch;
    dev_buf<uint64_t> dec_roff;
    // LPN PRF key material (SecKey) and pk.H_digest
    uint64_t prf_k[4] = {0, 0, 0, 0};
    dev_buf<uint64_t> lpn_s;
    uint32_t lpn_words = 0, lpn_t = 0, tau_num = 0, tau_den = 0;
    bool have_secret = false;
    uint8_t H_digest[32] = {0};
    bool have_digest = false;
    bool aes_tables = false;
    dev_buf<uint8_t> prf_req;
    dev_buf<uint64_t> prf_core;
    dev_buf<uint8_t> enc_arena;
    // general ct_mul path: host descriptors of the last plan, device copies, scratch arena
    std::vector<large_desc> large_host;   // the latest plan's pairs, in pair order
    sub_batch sub;                        // the sub-batch being launched (run_large)
    uint32_t plan_stamp = 0;
    uint64_t last_mul_pairs = 0;       // pairs of the last ct_mul_exec (pair_status is valid for these)
    uint64_t redo_total = 0;           // pairs re-run by redo_fresh_pairs since the context was created
    uint64_t path_total[4] = {};       // pair launches: fresh kernel, general path, its iblk order, direct mode
    double noise_bits = 120.0, noise_t2 = 0.55, noise_slope = 16.0;   // Params noise fields (enc plan_noise)
    dev_buf<large_desc> desc_dev;
    dev_buf<uint32_t> sel_dev;         // products: descriptor order per sub-batch (sub_batch::sel)
    dev_buf<uint32_t> arena;           // in 32-bit words
    // static bucket-group tables of the last plan (one per distinct bucket count) + build scratch
    dev_buf<uint32_t> grp, grp_tmp;
    dev_buf<uint32_t> salt_pos;
    dev_buf<mul_fresh_args> fresh_args;     // device copy of the fresh kernel's arguments
    mul_fresh_args fresh_args_host{};
    bool fresh_args_uploaded = false;       // the device copy holds fresh_args_host
    bool redo_cnt_dirty = true;             // redo_cnt may be nonzero (zeroed before the next exec)
    dev_buf<uint64_t> scan_scratch;
    dev_buf<plan_stats> stats;
    dev_buf<unsigned int> check_buf;     // gsum check: 4 layer maxima, then a u64 failure count
    dev_buf<uint8_t> check_scratch;      // gsum check: layer tables beyond LDS (global slabs)
    unsigned long long* totals = nullptr;   // [2]: &stats->total_layers (layer and edge slot totals), not owned
    void* pin = nullptr;   // pinned host words for the plan's and exec's read-backs (hipHostFree in ctx_destroy)
    sigma_tables H;
    // timing
    bool timing = false;
    std::map<std::string, timer_rec> timers;
    std::vector<hipEvent_t> ev_pool;   // timer events returned by flush_timers, reused (no create per launch)
    // general-path scratch cap in words (0 = half the free HBM): chain workers share the device
    uint64_t arena_cap_words = 0;
    dev_buf<uint64_t> img_tmp;         // image -> records: 3 words per edge of the pairs converted
    dev_buf<uint64_t> img_pairs;       // [2 n]: pair ids, then their offsets in img_tmp
    uint32_t img_grid_y = 65535;       // pairs per image -> records launch (PVAC_CHAIN_IMG_BATCH2: 2)
    uint32_t spin_us = 50000;          // read_back's spin before a blocking wait (chain workers: 200)
    // pvac_hip_ct_mul_chain: worker contexts (own stream / arena), and a worker's own buffers
    std::vector<pvac_hip_ctx*> chain_kids;   // [range j * streams + w] of the last call's layout
    chain_set chain_bufs[2];
    chain_set chain_stage;                   // a worker's staged chunk inputs (another device, or STAGE)
    chain_set chain_stage_op;                // ... and its staged per-step operand (pvac_chain_opts::operands)
    dev_stream_buf<uint64_t> chain_nonces;
    dev_stream_buf<uint64_t> chain_salts;    // final-step salts (WITH_SIGMA)
    dev_stream_buf<uint64_t> chain_out;      // digests / counts of a chunk before the copy to X's device
    dev_buf<unsigned long long> chain_stats;     // [2 * PVAC_CHAIN_MAX_DEPTH + 1]: edges / products, image pair-steps
    std::vector<int64_t> chain_layout;          // the last call's (streams, chunk, n_devices, ordinals...)
    // ct_recrypt and its parts (k_recrypt.hip)
    dev_buf<uint32_t> ubk_perm;              // pk.ubk as a gather: perm[inv[src]] = src (set_ubk)
    bool have_ubk = false;
    std::vector<merge_pair_info> compact_host;   // the latest compact plan's ciphers above the LDS bound
    dev_buf<uint64_t> zero_n;                // zero words: the counts of the merge path's empty B
    uint64_t compact_path[2] = {};           // ciphers compacted by k_compact_small / by the merge path
    uint64_t check_path[2] = {};             // check_mul_gsum calls with the tables in LDS / in global slabs
    dev_buf<uint64_t> rc_idx;                // recrypt: per-iteration offset / count views and popcounts
    dev_buf<uint32_t> rc_ids;                // recrypt: cipher ids of a view
    struct recrypt_set {                     // recrypt: one of the two intermediate batches
        dev_buf<pvac_layer> layers;
        dev_buf<uint64_t> meta, w_lo, w_hi, sigma;
    } rc_buf[2];
    dev_buf<unsigned long long> commit_counter;   // commit_ct: the cipher index its lanes draw from
    uint64_t H_gen = 0;                      // bumped whenever H is set (a worker's copy follows it)
    uint64_t H_from = 0;                     // worker: the parent's H_gen its H copy was taken from
};

namespace {

int fail(pvac_hip_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

int hip_fail(pvac_hip_ctx* c, hipError_t e, const char* where) {
    if (e == hipSuccess) return PVAC_OK;
    std::string m = std::string(where) + ": " + hipGetErrorString(e);
    return fail(c, e == hipErrorOutOfMemory ? PVAC_ENOMEM : PVAC_EDEVICE, m);
}

struct scoped_timer {
    pvac_hip_ctx* c;
    timer_rec* rec = nullptr;
    hipEvent_t a{}, b{};
    scoped_timer(pvac_hip_ctx* ctx, const char* name) : c(ctx) {
        if (!c->timing) return;
        rec = &c->timers[name];
        a = take();
        b = take();
        hipEventRecord(a, c->stream);
    }
    hipEvent_t take() {
        hipEvent_t e{};
        if (!c->ev_pool.empty()) {
            e = c->ev_pool.back();
            c->ev_pool.pop_back();
        } else {
            hipEventCreate(&e);
        }
        return e;
    }
    ~scoped_timer() {
        if (!rec) return;
        hipEventRecord(b, c->stream);
        rec->pending.emplace_back(a, b);
    }
};

void flush_timers(pvac_hip_ctx* c) {
    for (auto& kv : c->timers) {
        for (auto& ev : kv.second.pending) {
            hipEventSynchronize(ev.second);
            float ms = 0;
            hipEventElapsedTime(&ms, ev.first, ev.second);
            kv.second.ms += ms;
            kv.second.launches += 1;
            c->ev_pool.push_back(ev.first);
            c->ev_pool.push_back(ev.second);
        }
        kv.second.pending.clear();
    }
}

// The short host waits of a plan (its totals) and of exec (the redo count): a blocking
// hipStreamSynchronize wakes tens of microseconds after the copy lands, so spin on hipStreamQuery
// (up to spin_us, then block) and read into pinned words (a pageable destination stages the copy).
// A caller's context spins up to 50 ms (one thread, the headline step); the chain's worker contexts
// (several threads per device) spin 200 us and then block, so they do not hold cores and the HIP
// runtime's locks while their kernels run.
hipError_t read_back(pvac_hip_ctx* c, void* dst, const void* src, size_t bytes) {
    if (c->pin && bytes <= 256) {
        hipError_t e = hipMemcpyAsync(c->pin, src, bytes, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) return e;
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            e = hipStreamQuery(c->stream);
            if (e != hipErrorNotReady) break;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(c->spin_us)) {
                e = hipStreamSynchronize(c->stream);
                break;
            }
        }
        if (e == hipSuccess) std::memcpy(dst, c->pin, bytes);
        return e;
    }
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e;
}

// the exclusive scans' scratch for n counts
int ensure_scan(pvac_hip_ctx* c, size_t n) {
    const size_t sw = scan_scratch_words(n);
    return hip_fail(c, c->scan_scratch.grow(sw, sw), "alloc scan scratch");
}

// the six per-pair arrays are grown together (redo_ids last: its capacity stands for all of them)
int ensure_pairs(pvac_hip_ctx* c, size_t n) {
    hipError_t e = hipSuccess;
    if (n > c->redo_ids.capacity()) {
        c->pair_class.release();
        c->pair_status.release();
        c->large_ids.release();
        c->large_info.release();
        c->redo_ids.release();
        c->fresh_recs.release();
        const size_t cap = std::max<size_t>(n, 1024);
        e = c->pair_class.grow(n, cap);
        if (e == hipSuccess) e = c->pair_status.grow(n, cap);
        if (e == hipSuccess) e = c->large_ids.grow(n, cap);
        if (e == hipSuccess) e = c->large_info.grow(8 * n, 8 * cap);   // 5 (mul) or 8 (add merge) words per pair
        if (e == hipSuccess) e = c->fresh_recs.grow(n, cap);
        if (e == hipSuccess) e = c->redo_ids.grow(n, cap);
    }
    if (e == hipSuccess) e = c->redo_cnt.grow(4, 4);
    if (e != hipSuccess) return hip_fail(c, e, "alloc pair scratch");
    return ensure_scan(c, n);
}

bool batch_ok(const pvac_ct_batch* X) {
    return X && (X->n == 0 || (X->l_off && X->l_cnt && X->e_off && X->e_cnt));
}

}  // namespace

// ==================================================================== ABI
extern "C" {

int pvac_hip_abi_version(void) { return PVAC_HIP_ABI_VERSION; }

int pvac_hip_ctx_create(int device, const pvac_hip_params* prm, pvac_hip_ctx** out) {
    if (!out || !prm) return PVAC_EINVAL;
    *out = nullptr;
    if (prm->B == 0 || prm->B > 65535 || prm->m_bits == 0 || prm->n_bits == 0) return PVAC_EINVAL;
    pvac_hip_ctx* c = new (std::nothrow) pvac_hip_ctx();
    if (!c) return PVAC_ENOMEM;
    c->device = device;
    c->prm = *prm;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { pvac_hip_ctx_destroy(c); return PVAC_EDEVICE; }
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        c->num_cus = cus;
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { pvac_hip_ctx_destroy(c); return PVAC_EDEVICE; }
    c->own_stream = true;
    std::vector<uint32_t> nb(kNbTableLen);
    std::vector<uint64_t> mg(kNbTableLen);
    for (uint32_t n = 0; n < kNbTableLen; ++n) {
        nb[n] = (uint32_t)bucket_count_after_reserve(n);
        mg[n] = make_fastmod64(nb[n]).m;
        if (nb[n] == 0 || nb[n] > 0xFFFFu) { pvac_hip_ctx_destroy(c); return PVAC_ERANGE; }   // fresh_rec.nbk is u16
    }
    e = c->nb_table.grow(nb.size(), nb.size());
    if (e == hipSuccess) e = hipMemcpy(c->nb_table.get(), nb.data(), nb.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = c->nb_magic.grow(mg.size(), mg.size());
    if (e == hipSuccess) e = hipMemcpy(c->nb_magic.get(), mg.data(), mg.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = c->stats.grow(1, 1);
    // the scans' two totals are plan_stats' first words: a plan reads stats and totals back in one copy
    if (e == hipSuccess) c->totals = &c->stats.get()->total_layers;
    if (e == hipSuccess) e = hipHostMalloc(&c->pin, 256, hipHostMallocDefault);
    if (e != hipSuccess) { pvac_hip_ctx_destroy(c); return PVAC_ENOMEM; }
    *out = c;
    return PVAC_OK;
}

// a context's stream-ordered buffers (a chain worker's output batches, nonce / salt / result words)
// go back on its stream; the caller synchronises
static void release_stream_ordered(pvac_hip_ctx* c) {
    for (chain_set* b : {&c->chain_bufs[0], &c->chain_bufs[1], &c->chain_stage, &c->chain_stage_op}) b->release(c->stream);
    c->chain_nonces.release(c->stream);
    c->chain_salts.release(c->stream);
    c->chain_out.release(c->stream);
}

// everything a chain worker grew during a call (the above, image scratch, the general-path arena,
// the gsum check's slabs); the caller selected the worker's device
static hipError_t release_chain_worker(pvac_hip_ctx* k) {
    release_stream_ordered(k);
    const hipError_t e = hipStreamSynchronize(k->stream);
    k->img_tmp.release();
    k->img_pairs.release();
    k->arena.release();
    k->check_scratch.release();
    return e;
}

// The only deleter of a context (ctx_create's failure exits included): workers first, then this
// context's device, its stream drained, timer events, the stream-ordered buffers while the stream
// lives, the stream itself; the members' destructors free the rest before the caller's device returns.
int pvac_hip_ctx_destroy(pvac_hip_ctx* c) {
    if (!c) return PVAC_OK;
    for (pvac_hip_ctx* k : c->chain_kids) pvac_hip_ctx_destroy(k);
    device_guard dev(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    flush_timers(c);
    for (hipEvent_t e : c->ev_pool) hipEventDestroy(e);
    release_stream_ordered(c);
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

int pvac_hip_ctx_synchronize(pvac_hip_ctx* c) {
    if (!c) return PVAC_EINVAL;
    return hip_fail(c, hipStreamSynchronize(c->stream), "synchronize");
}

int pvac_hip_ct_mul_redo_count(pvac_hip_ctx* c, uint64_t* out) {
    if (!c || !out) return PVAC_EINVAL;
    *out = c->redo_total;
    return PVAC_OK;
}

int pvac_hip_ctx_set_noise(pvac_hip_ctx* c, double noise_entropy_bits, double tuple2_fraction, double depth_slope_bits) {
    if (!c || !(noise_entropy_bits >= 0.0) || !(tuple2_fraction >= 0.0 && tuple2_fraction <= 1.0) ||
        !(depth_slope_bits >= 0.0) || noise_entropy_bits > 1e6 || depth_slope_bits > 1e6)
        return fail(c, PVAC_EINVAL, "ctx_set_noise: noise_entropy_bits, depth_slope_bits >= 0, tuple2_fraction in [0, 1]");
    c->noise_bits = noise_entropy_bits;
    c->noise_t2 = tuple2_fraction;
    c->noise_slope = depth_slope_bits;
    return PVAC_OK;
}

int pvac_hip_ct_mul_path_count(pvac_hip_ctx* c, uint64_t* out) {
    if (!c || !out) return PVAC_EINVAL;
    for (int k = 0; k < 4; ++k) out[k] = c->path_total[k];
    return PVAC_OK;
}

int pvac_hip_ct_mul_status(pvac_hip_ctx* c, uint32_t* out, size_t n) {
    if (!c || (!out && n)) return fail(c, PVAC_EINVAL, "ct_mul_status: bad arguments");
    if (!n) return PVAC_OK;
    if (n > c->last_mul_pairs) return fail(c, PVAC_EINVAL, "ct_mul_status: more pairs than the last ct_mul_exec held");
    const hipError_t e = hipMemcpyAsync(out, c->pair_status.get(), n * 4, hipMemcpyDeviceToDevice, c->stream);
    return e == hipSuccess ? PVAC_OK : hip_fail(c, e, "ct_mul_status");
}

const char* pvac_hip_last_error(pvac_hip_ctx* c) { return c ? c->err.c_str() : "null context"; }

int pvac_hip_timing_enable(pvac_hip_ctx* c, int on) {
    if (!c) return PVAC_EINVAL;
    c->timing = on != 0;
    // events for the launches to come, created now rather than inside the timed launches
    while (c->timing && c->ev_pool.size() < 256) {
        hipEvent_t e{};
        if (hipEventCreate(&e) != hipSuccess) break;
        c->ev_pool.push_back(e);
    }
    return PVAC_OK;
}

int pvac_hip_timing_get(pvac_hip_ctx* c, const char* name, double* ms, uint64_t* launches) {
    if (!c || !name) return PVAC_EINVAL;
    flush_timers(c);
    auto it = c->timers.find(name);
    if (ms) *ms = it == c->timers.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == c->timers.end() ? 0 : it->second.launches;
    return PVAC_OK;
}

int pvac_hip_timing_reset(pvac_hip_ctx* c) {
    if (!c) return PVAC_EINVAL;
    flush_timers(c);
    c->timers.clear();
    return PVAC_OK;
}

// ---------------------------------------------------------------- Fp
int pvac_hip_fp_binop(pvac_hip_ctx* c, int op, const uint64_t* a_lo, const uint64_t* a_hi, const uint64_t* b_lo,
                      const uint64_t* b_hi, uint64_t* c_lo, uint64_t* c_hi, size_t n) {
    if (!c) return PVAC_EINVAL;
    if (op < PVAC_FP_ADD || op > PVAC_FP_INV) return fail(c, PVAC_EINVAL, "fp_binop: bad op");
    if (n && (!a_lo || !a_hi || !c_lo || !c_hi)) return fail(c, PVAC_EINVAL, "fp_binop: null array");
    if (n && op != PVAC_FP_NEG && op != PVAC_FP_INV && (!b_lo || !b_hi)) return fail(c, PVAC_EINVAL, "fp_binop: null b");
    scoped_timer t(c, "fp_binop");
    return hip_fail(c, launch_fp_binop(op, a_lo, a_hi, b_lo, b_hi, c_lo, c_hi, n, c->stream), "fp_binop");
}

// ---------------------------------------------------------------- ct_mul
namespace {

// Pairs whose bucket count is at least twice their key-slot space (dense chain steps: reserve(|A.E||B.E|)
// buckets for |A.L||B.L|B slots) share their bucket groups with every pair of the same bucket count:
// the group of a slot depends only on (slot, B, bucket count). One static table per distinct bucket
// count replaces the per-pair bucket table + chains (k_large_link) and its zeroing; rank walks the
// static group and keeps the slots present in the pair (almost every slot is alone in its bucket).
// Builds the tables of `set` into the context's one buffer (c->grp: they replace those of any other
// set) and rebuilds the descriptors of its pairs that use them; allow_direct = false keeps every
// pair on the full layout (per-key sums: the redo run, the canonical order).
int assign_static_groups(pvac_hip_ctx* c, std::vector<large_desc>& set, bool allow_direct) {
    constexpr size_t kMaxCfg = 64;
    constexpr uint64_t kMaxWords = 1ull << 28;   // <= 1 GiB of tables
    std::map<uint64_t, uint64_t> cfg;             // bucket count -> max S
    for (const large_desc& d : set)
        if (d.nbm.d >= 2 * d.S && d.S) {
            uint64_t& m = cfg[d.nbm.d];
            m = std::max(m, d.S);
        }
    uint64_t words = 0, tmp_max = 0;
    for (auto& kv : cfg) {
        words += 2 * kv.second;
        tmp_max = std::max<uint64_t>(tmp_max, 1ull << std::max<uint32_t>(1, ceil_log2(2 * kv.second)));
    }
    if (cfg.empty() || cfg.size() > kMaxCfg || words > kMaxWords) return PVAC_OK;   // dynamic chains
    int rc = hip_fail(c, c->grp.grow_floor(words), "alloc bucket-group tables");
    if (!rc) rc = hip_fail(c, c->grp_tmp.grow_floor(3 * tmp_max), "alloc bucket-group scratch");
    if (rc) return rc;
    std::map<uint64_t, uint64_t> off;   // bucket count -> head offset (next = head + S_max)
    uint64_t o = 0;
    for (auto& kv : cfg) {
        const uint64_t Sm = kv.second;
        const uint32_t hb = std::max<uint32_t>(1, ceil_log2(2 * Sm));
        const uint64_t hcap = 1ull << hb;
        unsigned long long* tk = (unsigned long long*)c->grp_tmp.get();   // [hcap] u64 keys, then [hcap] u32 heads
        uint32_t* th = c->grp_tmp.get() + 2 * hcap;
        hipError_t e = hipMemsetAsync(c->grp_tmp.get(), 0, 3 * hcap * 4, c->stream);
        if (e == hipSuccess)
            e = launch_grp_build(make_fastmod64(kv.first), c->prm.B, Sm, hb, c->grp.get() + o, c->grp.get() + o + Sm, tk, th,
                                 c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "build bucket-group tables");
        off[kv.first] = o;
        o += 2 * Sm;
    }
    for (large_desc& d : set) {
        auto it = off.find(d.nbm.d);
        if (it == off.end() || d.nbm.d < 2 * d.S || !d.S) continue;
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
    hipError_t e = launch_gather_large(*A, *B, ids, n, c->large_info.get(), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(info.data(), c->large_info.get(), info.size() * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, where);
    out.resize(n);
    for (uint64_t k = 0; k < n; ++k) {
        std::string why;
        const int rc = build_large_desc(out[k], info[5 * k], info[5 * k + 1], info[5 * k + 2], info[5 * k + 3],
                                        info[5 * k + 4], c->prm.B, why);
        if (rc) {
            out.clear();
            return fail(c, rc, why);
        }
    }
    std::sort(out.begin(), out.end(), [](const large_desc& x, const large_desc& y) { return x.pair < y.pair; });
    return PVAC_OK;
}

}  // namespace

int pvac_hip_ct_mul_plan(pvac_hip_ctx* c, const pvac_ct_batch* A, const pvac_ct_batch* B, pvac_ct_batch* C,
                         pvac_hip_plan* plan) {
    if (!c || !plan || !batch_ok(A) || !batch_ok(B) || !C || !C->l_off || !C->e_off)
        return fail(c, PVAC_EINVAL, "ct_mul_plan: bad arguments");
    if (A->n != B->n) return fail(c, PVAC_EINVAL, "ct_mul_plan: |A| != |B|");
    std::memset(plan, 0, sizeof *plan);
    plan->kind = 1;
    plan->n_pairs = A->n;
    C->n = A->n;
    c->large_host.clear();
    // every earlier plan goes stale now; this one is stamped valid only once it has succeeded, so
    // exec rejects a plan whose device work or descriptor build failed
    const uint32_t stamp = ++c->plan_stamp;
    if (!A->n) {
        plan->reserved[0] = stamp;
        return PVAC_OK;
    }
    int rc = ensure_pairs(c, A->n);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync(c->stats.get(), 0, sizeof(plan_stats), c->stream);
    if (e == hipSuccess)
        e = launch_plan_mul(*A, *B, *C, c->pair_class.get(), c->large_ids.get(), c->stats.get(), c->nb_table.get(), kNbTableLen, c->prm.B,
                            c->stream);
    if (e == hipSuccess)
        e = launch_exclusive_scan2_u64(C->l_off, C->e_off, A->n, c->scan_scratch.get(), &c->totals[0], &c->totals[1], c->stream);
    plan_stats st{};
    if (e == hipSuccess) e = read_back(c, &st, c->stats.get(), sizeof st);
    const unsigned long long tot[2] = {st.total_layers, st.total_edges};
    if (e != hipSuccess) return hip_fail(c, e, "ct_mul_plan");
    plan->total_layer_slots = tot[0];
    plan->total_edge_slots = tot[1];
    plan->n_small = A->n - st.n_large;   // k_plan_mul classifies every pair as small or large
    plan->n_large = st.n_large;
    plan->max_keys = st.max_keys;
    plan->max_prod = st.max_prod;
    plan->max_na = st.max_na;
    plan->max_nb = st.max_nb;
    plan->max_buckets = st.max_buckets;
    plan->max_layers = st.max_layers;
    if (st.n_large) {
        rc = gather_large_descs(c, A, B, c->large_ids.get(), st.n_large, c->large_host, "ct_mul_plan (large)");
        if (!rc) rc = assign_static_groups(c, c->large_host, true);
        if (rc) {
            c->large_host.clear();
            return rc;
        }
    }
    plan->reserved[0] = stamp;
    return PVAC_OK;
}

namespace {

// A chain step's dense images (pvac_hip_ct_mul_chain; mul_large_args::A_img / C_img): per-pair flags
// of A (read; cleared where A is turned back into records) and of C (written), and the counter of
// pair-steps written as images. All null outside the chain.
struct step_images {
    uint32_t* in = nullptr;
    uint32_t* out = nullptr;
    unsigned long long* count = nullptr;
};

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
    int rc = hip_fail(c, c->img_pairs.grow_floor(h.size()), "alloc image pairs");
    if (!rc) rc = hip_fail(c, c->img_tmp.grow_floor(3 * std::max<uint64_t>(tot, 1)), "alloc image scratch");
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(c->img_pairs.get(), h.data(), h.size() * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = launch_image_to_records(*A, img.in, c->img_pairs.get(), (uint32_t)pn.size(), c->img_tmp.get(), c->prm.B,
                                    c->img_grid_y, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // h is read from the host stack
    return e == hipSuccess ? PVAC_OK : hip_fail(c, e, "chain images to records");
}

// Runs the general path over `set` (pair order, static groups assigned) in sub-batches that fit the
// scratch budget (cut_sub_batch, large_plan.hpp).
int run_large(pvac_hip_ctx* c, const std::vector<large_desc>& set, const pvac_ct_batch* A, const pvac_ct_batch* B,
              const uint64_t* nonces, pvac_ct_batch* C, uint32_t flags, uint32_t* salt_pos, step_images img) {
    const size_t nl = set.size();
    int rc = hip_fail(c, c->desc_dev.grow_floor(nl), "alloc large descriptors");
    if (!rc) rc = hip_fail(c, c->sel_dev.grow_floor(nl), "alloc large descriptor order");
    if (rc) return rc;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 8ull << 30;
    uint64_t budget = std::max<uint64_t>((uint64_t)(free_b / 2) / 4 + c->arena.capacity(), 1ull << 24);
    budget = std::min<uint64_t>(budget, 16ull << 30);   // <= 64 GiB of scratch per sub-batch
    // a worker of pvac_hip_ct_mul_chain shares the device with the other workers: its share
    if (c->arena_cap_words) budget = std::min<uint64_t>(budget, std::max<uint64_t>(c->arena_cap_words, c->arena.capacity()));
    sub_batch& sb = c->sub;
    size_t i = 0;
    while (i < nl) {
        // the uploads below read sb's vectors when the stream reaches them: the previous sub-batch's
        // must have been taken before its storage is cut anew
        if (i && hipStreamSynchronize(c->stream) != hipSuccess) return hip_fail(c, hipErrorUnknown, "ct_mul_large");
        cut_sub_batch(set, i, budget, sb);
        if (sb.words > c->arena.capacity()) {
            // grow with 1/8 headroom (within the budget): batches of similar pairs differ by a few
            // words, and a free + re-malloc of tens of GB stalls for seconds
            uint64_t grown = std::max<uint64_t>(sb.words, std::min<uint64_t>(sb.words + sb.words / 8, budget));
            hipStreamSynchronize(c->stream);
            const auto t0 = std::chrono::steady_clock::now();
            hipError_t e = c->arena.grow(sb.words, grown);   // frees the old arena first
            if (e == hipErrorOutOfMemory && grown > sb.words) {   // without the headroom
                (void)hipGetLastError();
                grown = sb.words;
                e = c->arena.grow(sb.words, grown);
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
        hipError_t e = hipMemcpyAsync(c->desc_dev.get() + i, sb.desc.data(), sb.desc.size() * sizeof(large_desc),
                                      hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(c->sel_dev.get() + i, sb.sel.data(), sb.sel.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                               c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "upload large descriptors");
        mul_large_args a = sb.sizing;
        a.A = *A; a.B = *B; a.C = *C;
        a.nonces = nonces;
        a.pair_status = c->pair_status.get();
        a.desc = c->desc_dev.get() + i;
        a.scratch = c->arena.get();
        a.Bm = c->prm.B;
        a.canon_tag = c->prm.canon_tag;
        a.edge_budget = c->prm.edge_budget;
        a.flags = flags;
        a.salt_pos = salt_pos;
        a.grp = c->grp.get();
        a.sel = c->sel_dev.get() + i;
        a.redo_ids = c->redo_ids.get();
        a.redo_cnt = c->redo_cnt.get();
        a.A_img = img.in;
        a.C_img = img.out;
        a.img_count = img.out ? img.count : nullptr;
        e = launch_ct_mul_large(a, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "ct_mul_large");
        c->path_total[1] += sb.end - i;
        c->path_total[2] += sb.n_iblk;
        c->path_total[3] += sb.n_direct;
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
    hipError_t e = read_back(c, &cnt, c->redo_cnt.get(), sizeof cnt);
    if (e != hipSuccess) return hip_fail(c, e, "ct_mul_exec (redo count)");
    if (!cnt) {
        c->redo_cnt_dirty = false;
        return PVAC_OK;
    }
    std::vector<large_desc> redo;
    int rc = gather_large_descs(c, A, B, c->redo_ids.get(), cnt, redo, "ct_mul_exec (redo shapes)");
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
        c->redo_total += cnt;
        if (!c->large_host.empty()) rc = assign_static_groups(c, c->large_host, true);
    }
    // on failure the group tables may still belong to the redo set: no exec may reuse this plan
    if (rc) ++c->plan_stamp;
    return rc;
}

// pvac_hip_ct_mul_exec, with a chain step's images (all null for a caller's batch)
int ct_mul_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* A, const pvac_ct_batch* B,
                const uint64_t* nonces, const uint64_t* salts, pvac_ct_batch* C, uint32_t flags, step_images img) {
    if (!c || !plan || plan->kind != 1 || !batch_ok(A) || !batch_ok(B) || !batch_ok(C))
        return fail(c, PVAC_EINVAL, "ct_mul_exec: bad arguments");
    if (A->n != plan->n_pairs || B->n != plan->n_pairs) return fail(c, PVAC_EINVAL, "ct_mul_exec: plan mismatch");
    if (!A->n) return PVAC_OK;
    if (plan->reserved[0] != c->plan_stamp || plan->n_large != c->large_host.size())
        return fail(c, PVAC_EINVAL, "ct_mul_exec: plan is not this context's latest ct_mul plan");
    if (!nonces) return fail(c, PVAC_EINVAL, "ct_mul_exec: nonces required");
    if (!C->layers || !C->meta || !C->w_lo || !C->w_hi) return fail(c, PVAC_EINVAL, "ct_mul_exec: output arrays");
    c->last_mul_pairs = 0;   // pair_status is valid again only once this exec has launched its kernels
    const bool with_sigma = (flags & PVAC_MUL_WITH_SIGMA) != 0;
    if (with_sigma && (!salts || !C->sigma || !c->H.ready))
        return fail(c, PVAC_EINVAL, "ct_mul_exec: WITH_SIGMA needs salts, C->sigma and H");
    uint32_t* salt_pos = nullptr;
    if (with_sigma) {
        int rc = hip_fail(c, c->salt_pos.grow_floor(plan->total_edge_slots), "alloc salt positions");
        if (rc) return rc;
        salt_pos = c->salt_pos.get();
    }
    if (c->redo_cnt_dirty) {   // a read-back of zero leaves it clean: no memset per exec
        const hipError_t e = hipMemsetAsync(c->redo_cnt.get(), 0, sizeof(unsigned int), c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "reset redo count");
    }
    c->redo_cnt_dirty = true;   // until this exec reads back a zero count
    c->path_total[0] += plan->n_small;
    if (plan->n_small) {
        mul_fresh_args a;
        std::memset(&a, 0, sizeof a);   // padding too: the upload below is skipped on equal bytes
        a.A = *A; a.B = *B; a.C = *C;
        a.recs = c->fresh_recs.get();
        a.nonces = nonces;
        a.pair_class = c->pair_class.get();
        a.pair_status = c->pair_status.get();
        a.nb_table = c->nb_table.get();
        a.nb_magic = c->nb_magic.get();
        a.salt_pos = salt_pos;
        a.redo_ids = c->redo_ids.get();
        a.redo_cnt = c->redo_cnt.get();
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
        if (const hipError_t ea = c->fresh_args.grow(1, 1)) return hip_fail(c, ea, "alloc fresh args");
        // stream-ordered copy from the ctx's host mirror (kept alive until the next exec); a batch
        // exec'd again into the same buffers (the kernels never write their arguments) reuses it
        hipError_t e = hipSuccess;
        if (!c->fresh_args_uploaded || std::memcmp(&c->fresh_args_host, &a, sizeof a) != 0) {
            c->fresh_args_uploaded = false;
            std::memcpy(&c->fresh_args_host, &a, sizeof a);
            e = hipMemcpyAsync(c->fresh_args.get(), &c->fresh_args_host, sizeof a, hipMemcpyHostToDevice, c->stream);
            c->fresh_args_uploaded = e == hipSuccess;
        }
        if (e != hipSuccess) return hip_fail(c, e, "upload fresh args");
        scoped_timer t(c, "ct_mul_fresh");
        e = launch_ct_mul_fresh(a, c->fresh_args.get(), c->num_cus, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "ct_mul_fresh");
    }
    if (plan->n_large && (flags & PVAC_MUL_ORDER_CANONICAL) &&
        std::any_of(c->large_host.begin(), c->large_host.end(), [](const large_desc& d) { return d.direct != 0; })) {
        // the direct mode emits hash order only: with the canonical order asked for, its pairs would
        // all be redone, so take them on the full layout from the start (descriptors rebuilt once;
        // the plan stays valid, its direct pairs now run the exact path)
        const int rc = assign_static_groups(c, c->large_host, false);
        if (rc) {
            ++c->plan_stamp;
            return rc;
        }
    }
    if (plan->n_large && img.in) {   // chain step: image inputs of pairs off the direct mode -> records
        std::vector<std::pair<uint64_t, uint64_t>> pn;
        for (const large_desc& d : c->large_host)
            if (!d.direct) pn.emplace_back(d.pair, d.nA);
        const int rc = images_to_records(c, A, pn, img);
        if (rc) return rc;
    }
    if (plan->n_large) {
        scoped_timer t(c, "ct_mul_large");
        int rc = run_large(c, c->large_host, A, B, nonces, C, flags, salt_pos, img);
        if (rc) return rc;
    }
    {
        int rc = redo_fresh_pairs(c, A, B, nonces, C, flags, salt_pos, img);
        if (rc) return rc;
    }
    c->last_mul_pairs = A->n;
    if (with_sigma) {
        scoped_timer t(c, "sigma");
        hipError_t e = launch_sigma(c->H, c->prm, *C, salts, salt_pos, c->num_cus, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "sigma");
    }
    return PVAC_OK;
}

}  // namespace

int pvac_hip_ct_mul_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* A, const pvac_ct_batch* B,
                         const uint64_t* nonces, const uint64_t* salts, pvac_ct_batch* C, uint32_t flags) {
    return ct_mul_exec(c, plan, A, B, nonces, salts, C, flags, {});
}

int pvac_hip_ct_mul(pvac_hip_ctx* c, const pvac_ct_batch* A, const pvac_ct_batch* B, pvac_ct_batch* C,
                    uint64_t layer_cap, uint64_t edge_cap, const uint64_t* nonces, const uint64_t* salts,
                    uint32_t flags, pvac_hip_plan* plan_out) {
    pvac_hip_plan p{};
    int rc = pvac_hip_ct_mul_plan(c, A, B, C, &p);
    if (plan_out) *plan_out = p;
    if (rc) return rc;
    if (p.total_layer_slots > layer_cap || p.total_edge_slots > edge_cap) {
        ++c->plan_stamp;   // the plan's offsets do not fit C: it is not exec'd
        return fail(c, PVAC_ENOMEM, "ct_mul: output capacity below the plan's totals");
    }
    return pvac_hip_ct_mul_exec(c, &p, A, B, nonces, salts, C, flags);
}

// ---------------------------------------------------------------- ct_add / ct_sub
int pvac_hip_ct_add_plan(pvac_hip_ctx* c, const pvac_ct_batch* A, const pvac_ct_batch* B, pvac_ct_batch* C,
                         pvac_hip_plan* plan) {
    if (!c || !plan || !batch_ok(A) || !batch_ok(B) || !C || !C->l_off || !C->e_off)
        return fail(c, PVAC_EINVAL, "ct_add_plan: bad arguments");
    if (A->n != B->n) return fail(c, PVAC_EINVAL, "ct_add_plan: |A| != |B|");
    std::memset(plan, 0, sizeof *plan);
    plan->kind = 2;
    plan->n_pairs = A->n;
    C->n = A->n;
    if (!A->n) return PVAC_OK;
    int rc = ensure_pairs(c, A->n);
    if (rc) return rc;
    c->merge_host.clear();
    // as in ct_mul_plan: earlier plans go stale now, this one is stamped only once it has succeeded
    const uint32_t stamp = ++c->plan_stamp;
    hipError_t e = hipMemsetAsync(c->stats.get(), 0, sizeof(plan_stats), c->stream);
    if (e == hipSuccess)
        e = launch_plan_add(*A, *B, *C, c->stats.get(), c->pair_class.get(), c->large_ids.get(), c->prm.edge_budget, c->stream);
    if (e == hipSuccess)
        e = launch_exclusive_scan2_u64(C->l_off, C->e_off, A->n, c->scan_scratch.get(), &c->totals[0], &c->totals[1], c->stream);
    plan_stats st{};
    if (e == hipSuccess) e = read_back(c, &st, c->stats.get(), sizeof st);
    const unsigned long long tot[2] = {st.total_layers, st.total_edges};
    if (e != hipSuccess) return hip_fail(c, e, "ct_add_plan");
    plan->total_layer_slots = tot[0];
    plan->total_edge_slots = tot[1];
    plan->max_layers = st.max_layers;
    plan->n_large = st.n_large;
    plan->n_small = A->n - st.n_large;
    if (st.n_large) {   // guard_budget pairs: shapes and offsets for the per-pair merge launches
        std::vector<uint64_t> info(8 * st.n_large);
        e = launch_gather_merge(*A, *B, *C, c->large_ids.get(), st.n_large, c->large_info.get(), c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(info.data(), c->large_info.get(), info.size() * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "ct_add_plan (merge)");
        for (uint64_t k = 0; k < st.n_large; ++k) {
            const uint64_t* o = &info[8 * k];
            merge_pair_info m{};
            m.pair = o[0];
            m.LA = (uint32_t)o[1];
            m.L = (uint32_t)(o[1] + o[2]);
            m.nA = o[3];
            m.nB = o[4];
            m.aeo = o[5];
            m.beo = o[6];
            m.ceo = o[7];
            if (m.nA + m.nB >= (1ull << 31) || (uint64_t)m.L * c->prm.B * 2 >= 0xFFFFFFFFull) {
                c->merge_host.clear();
                return fail(c, PVAC_ENOSYS, "ct_add_plan: over-budget pair beyond 2^31 edges or 2^32 keys");
            }
            c->merge_host.push_back(m);
        }
        std::sort(c->merge_host.begin(), c->merge_host.end(),
                  [](const merge_pair_info& x, const merge_pair_info& y) { return x.pair < y.pair; });
    }
    plan->reserved[0] = stamp;
    return PVAC_OK;
}

int pvac_hip_ct_add_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* A, const pvac_ct_batch* B,
                         int negate_b, pvac_ct_batch* C) {
    if (!c || !plan || plan->kind != 2 || !batch_ok(A) || !batch_ok(B) || !batch_ok(C))
        return fail(c, PVAC_EINVAL, "ct_add_exec: bad arguments");
    if (A->n != plan->n_pairs || B->n != plan->n_pairs) return fail(c, PVAC_EINVAL, "ct_add_exec: plan mismatch");
    if (!A->n) return PVAC_OK;
    if (plan->max_layers > 30000) return fail(c, PVAC_ENOSYS, "ct_add_exec: > 30000 layers per cipher");
    if (plan->n_large && (plan->reserved[0] != c->plan_stamp || plan->n_large != c->merge_host.size()))
        return fail(c, PVAC_EINVAL, "ct_add_exec: plan is not this context's latest plan");
    {
        scoped_timer t(c, "ct_add");
        const int rc = hip_fail(c,
                                launch_ct_add(*A, *B, *C, negate_b, plan->max_layers,
                                              plan->n_large ? c->pair_class.get() : nullptr, c->stream),
                                "ct_add");
        if (rc) return rc;
    }
    if (!plan->n_large) return PVAC_OK;
    // guard_budget (encrypt.hpp:106-111): compact_edges + compact_layers per over-budget pair
    scoped_timer t(c, "ct_add_merge");
    if (const hipError_t e = c->merge_counters.grow(2, 2)) return hip_fail(c, e, "alloc merge counters");
    for (const merge_pair_info& m : c->merge_host) {
        const size_t need = merge_scratch_bytes(m.nA + m.nB, m.L);
        if (const hipError_t e = c->merge_scratch.grow(need, need)) return hip_fail(c, e, "alloc merge scratch");
        const int rc = hip_fail(c,
                                launch_add_merge(*A, *B, *C, m.pair, m, c->prm.B, negate_b, c->merge_scratch.get(),
                                                 c->merge_scratch.capacity(), c->merge_counters.get(), c->stream),
                                "ct_add merge");
        if (rc) return rc;
    }
    return PVAC_OK;
}

int pvac_hip_ct_scale(pvac_hip_ctx* c, pvac_ct_batch* X, uint64_t s_lo, uint64_t s_hi) {
    if (!c || !batch_ok(X)) return PVAC_EINVAL;
    scoped_timer t(c, "ct_scale");
    return hip_fail(c, launch_ct_scale(*X, s_lo, s_hi, c->stream), "ct_scale");
}

// ---------------------------------------------------------------- sigma / H
int pvac_hip_ctx_set_H(pvac_hip_ctx* c, const uint64_t* H, uint32_t n_cols, uint32_t wpc) {
    if (!c || !H) return PVAC_EINVAL;
    if (n_cols != c->prm.n_bits || wpc != (c->prm.m_bits + 63) / 64) return fail(c, PVAC_EINVAL, "set_H: shape");
    try {
        const int rc = hip_fail(c, sigma_tables_from_dense(c->H, c->prm, H, c->stream), "set_H");
        if (rc) return rc;
        ++c->H_gen;
        // H_digest = SHA-256("H|v2" || le64 m || le64 n || le64 wt || column bytes) (matrix.hpp:218-250)
        const size_t colbytes = (c->prm.m_bits + 7) / 8;
        std::vector<uint8_t> msg(28 + (size_t)n_cols * colbytes);
        std::memcpy(msg.data(), "H|v2", 4);
        const uint64_t hdr[3] = {c->prm.m_bits, c->prm.n_bits, c->prm.h_col_wt};
        for (int k = 0; k < 3; ++k)
            for (int i = 0; i < 8; ++i) msg[4 + 8 * k + i] = (uint8_t)(hdr[k] >> (8 * i));
        for (uint32_t col = 0; col < n_cols; ++col)
            for (size_t b = 0; b < colbytes; ++b)
                msg[28 + (size_t)col * colbytes + b] = (uint8_t)(H[(size_t)col * wpc + b / 8] >> (8 * (b % 8)));
        sha256_host(msg.data(), msg.size(), c->H_digest);
        c->have_digest = true;
        return PVAC_OK;
    } catch (const std::exception& ex) {
        return fail(c, PVAC_ENOMEM, std::string("set_H: ") + ex.what());
    }
}

int pvac_hip_ctx_gen_H(pvac_hip_ctx* c, uint8_t digest[32]) {
    if (!c) return PVAC_EINVAL;
    try {
        scoped_timer t(c, "gen_H");
        uint8_t d[32];
        const int rc = hip_fail(c, sigma_tables_generate(c->H, c->prm, d, c->stream), "gen_H");
        if (rc) return rc;
        ++c->H_gen;
        std::memcpy(c->H_digest, d, 32);
        c->have_digest = true;
        if (digest) std::memcpy(digest, d, 32);
        return PVAC_OK;
    } catch (const std::exception& ex) {
        return fail(c, PVAC_ENOMEM, std::string("gen_H: ") + ex.what());
    }
}

int pvac_hip_sigma_batch(pvac_hip_ctx* c, pvac_ct_batch* X, const uint64_t* salts) {
    if (!c || !batch_ok(X) || !salts || !X->sigma) return PVAC_EINVAL;
    if (!c->H.ready) return fail(c, PVAC_EINVAL, "sigma_batch: H not set");
    scoped_timer t(c, "sigma");
    return hip_fail(c, launch_sigma(c->H, c->prm, *X, salts, nullptr, c->num_cus, c->stream), "sigma");
}

// ---------------------------------------------------------------- ct_recrypt and its parts
int pvac_hip_ctx_set_ubk(pvac_hip_ctx* c, const int32_t* inv, uint32_t m_bits) {
    if (!c || !inv) return fail(c, PVAC_EINVAL, "set_ubk: arguments");
    if (m_bits != c->prm.m_bits) return fail(c, PVAC_EINVAL, "set_ubk: m_bits is not the context's");
    try {
        // the kernel gathers: output bit j = input bit perm[j], perm[inv[src]] = src
        std::vector<uint32_t> perm(m_bits, 0xFFFFFFFFu);
        for (uint32_t s = 0; s < m_bits; ++s) {
            const int32_t j = inv[s];
            if (j < 0 || (uint32_t)j >= m_bits || perm[j] != 0xFFFFFFFFu)
                return fail(c, PVAC_EINVAL, "set_ubk: inv is not a permutation of [0, m_bits)");
            perm[j] = s;
        }
        hipError_t e = hipStreamSynchronize(c->stream);   // an earlier ubk_apply may still read the table
        if (e == hipSuccess) e = c->ubk_perm.grow(m_bits, m_bits);
        if (e == hipSuccess) e = hipMemcpy(c->ubk_perm.get(), perm.data(), (size_t)m_bits * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(c, e, "set_ubk");
        c->have_ubk = true;
        return PVAC_OK;
    } catch (const std::exception& ex) {
        return fail(c, PVAC_ENOMEM, std::string("set_ubk: ") + ex.what());
    }
}

namespace {

bool sigma_ok(const pvac_hip_ctx* c, const pvac_ct_batch* X) {
    return X->sigma && X->sigma_words >= (c->prm.m_bits + 63) / 64;
}

// compact's plan: the class of every cipher of X (pair_class), the ciphers above the LDS bound
// (compact_host, with C's edge offsets) and, with `scan`, C's offsets as the scans of X's counts
int compact_classify(pvac_hip_ctx* c, const pvac_ct_batch* X, pvac_ct_batch* C, bool scan, pvac_hip_plan* plan) {
    std::memset(plan, 0, sizeof *plan);
    plan->kind = 5;
    plan->n_pairs = X->n;
    c->compact_host.clear();
    if (!X->n) return PVAC_OK;
    if (X->n > 0x7FFFFFFFull) return fail(c, PVAC_ENOSYS, "compact: more than 2^31 - 1 ciphers");
    const int rc = ensure_pairs(c, X->n);
    if (rc) return rc;
    const uint32_t stamp = ++c->plan_stamp;   // earlier plans go stale now (pair_class is shared)
    pvac_ct_batch Cw = *C;
    if (!scan) Cw.l_off = Cw.e_off = nullptr;
    hipError_t e = hipMemsetAsync(c->stats.get(), 0, sizeof(plan_stats), c->stream);
    if (e == hipSuccess)
        e = launch_compact_plan(*X, Cw, c->prm.B, c->pair_class.get(), c->large_ids.get(), c->stats.get(), c->stream);
    if (e == hipSuccess && scan)
        e = launch_exclusive_scan2_u64(C->l_off, C->e_off, X->n, c->scan_scratch.get(), &c->totals[0], &c->totals[1], c->stream);
    plan_stats st{};
    if (e == hipSuccess) e = read_back(c, &st, c->stats.get(), sizeof st);
    if (e != hipSuccess) return hip_fail(c, e, "compact_plan");
    plan->total_layer_slots = st.total_layers;
    plan->total_edge_slots = st.total_edges;
    plan->max_layers = st.max_layers;
    plan->max_keys = st.max_keys;
    plan->n_large = st.n_large;
    plan->n_small = X->n - st.n_large;
    if (st.n_large) {
        std::vector<uint64_t> info(8 * st.n_large);
        e = launch_compact_gather(*X, *C, c->large_ids.get(), st.n_large, c->large_info.get(), c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(info.data(), c->large_info.get(), info.size() * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "compact_plan (merge)");
        for (uint64_t k = 0; k < st.n_large; ++k) {
            const uint64_t* o = &info[8 * k];
            merge_pair_info m{};
            m.pair = o[0];
            m.LA = m.L = (uint32_t)o[1];
            m.nA = o[2];
            m.nB = 0;
            m.aeo = o[3];
            m.beo = 0;
            m.ceo = o[4];
            if (o[1] > 30000 || m.nA >= (1ull << 31) || o[1] * c->prm.B * 2 >= 0xFFFFFFFFull) {
                c->compact_host.clear();
                return fail(c, PVAC_ENOSYS, "compact_plan: a cipher beyond 30000 layers, 2^31 edges or 2^32 keys");
            }
            c->compact_host.push_back(m);
        }
        std::sort(c->compact_host.begin(), c->compact_host.end(),
                  [](const merge_pair_info& x, const merge_pair_info& y) { return x.pair < y.pair; });
    }
    plan->reserved[0] = stamp;
    return PVAC_OK;
}

int compact_execute(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* X, pvac_ct_batch* C) {
    if (!X->n) return PVAC_OK;
    if (plan->reserved[0] != c->plan_stamp || plan->n_large != c->compact_host.size())
        return fail(c, PVAC_EINVAL, "compact_exec: plan is not this context's latest plan");
    scoped_timer t(c, "compact");
    if (plan->n_small) {
        const int rc = hip_fail(c,
                                launch_compact_small(*X, *C, c->pair_class.get(), c->prm.B, c->prm.m_bits, plan->max_keys,
                                                     c->stream),
                                "compact");
        if (rc) return rc;
        c->compact_path[0] += plan->n_small;
    }
    if (!plan->n_large) return PVAC_OK;
    // the merge path of ct_add's guard_budget (k_add_merge.hip), one cipher at a time, with an empty B
    hipError_t e = c->zero_n.grow(X->n, std::max<size_t>(X->n, 1024));
    if (e == hipSuccess) e = hipMemsetAsync(c->zero_n.get(), 0, X->n * 8, c->stream);
    if (e == hipSuccess) e = c->merge_counters.grow(2, 2);
    if (e != hipSuccess) return hip_fail(c, e, "alloc compact merge");
    pvac_ct_batch Bz = *X;
    Bz.l_off = Bz.l_cnt = Bz.e_off = Bz.e_cnt = c->zero_n.get();
    for (const merge_pair_info& m : c->compact_host) {
        const size_t need = merge_scratch_bytes(m.nA, m.L);
        if ((e = c->merge_scratch.grow(need, need)) != hipSuccess) return hip_fail(c, e, "alloc merge scratch");
        const int rc = hip_fail(c,
                                launch_add_merge(*X, Bz, *C, m.pair, m, c->prm.B, 0, c->merge_scratch.get(),
                                                 c->merge_scratch.capacity(), c->merge_counters.get(), c->stream),
                                "compact merge");
        if (rc) return rc;
    }
    c->compact_path[1] += plan->n_large;
    return PVAC_OK;
}

// n words to the device on the context's stream, waited for: the host words may change afterwards
hipError_t upload_words(pvac_hip_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!bytes) return hipSuccess;
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e;
}

}  // namespace

int pvac_hip_sigma_popcount(pvac_hip_ctx* c, const pvac_ct_batch* X, uint64_t* ones) {
    if (!c || !batch_ok(X) || (!ones && X->n)) return fail(c, PVAC_EINVAL, "sigma_popcount: bad arguments");
    if (!X->n) return PVAC_OK;
    if (!sigma_ok(c, X)) return fail(c, PVAC_EINVAL, "sigma_popcount: X carries no sigma of m_bits");
    if (X->n > 0x7FFFFFFFull) return fail(c, PVAC_ENOSYS, "sigma_popcount: more than 2^31 - 1 ciphers");
    scoped_timer t(c, "sigma_popcount");
    return hip_fail(c, launch_sigma_popcount(*X, c->prm.m_bits, c->num_cus, (unsigned long long*)ones, c->stream),
                    "sigma_popcount");
}

int pvac_hip_ubk_apply(pvac_hip_ctx* c, pvac_ct_batch* X, const uint32_t* active) {
    if (!c || !batch_ok(X)) return fail(c, PVAC_EINVAL, "ubk_apply: bad arguments");
    if (!c->have_ubk) return fail(c, PVAC_EINVAL, "ubk_apply: set_ubk first");
    if (!X->n) return PVAC_OK;
    if (!sigma_ok(c, X)) return fail(c, PVAC_EINVAL, "ubk_apply: X carries no sigma of m_bits");
    if (ubk_apply_lds_bytes(c->prm.m_bits) > 64 * 1024) return fail(c, PVAC_ENOSYS, "ubk_apply: m_bits beyond the LDS table");
    scoped_timer t(c, "ubk_apply");
    return hip_fail(c, launch_ubk_apply(*X, c->ubk_perm.get(), c->prm.m_bits, active, c->num_cus, c->stream), "ubk_apply");
}

int pvac_hip_compact_plan(pvac_hip_ctx* c, const pvac_ct_batch* X, pvac_ct_batch* C, pvac_hip_plan* plan) {
    if (!c || !plan || !batch_ok(X) || !C || (X->n && (!C->l_off || !C->e_off)))
        return fail(c, PVAC_EINVAL, "compact_plan: bad arguments");
    if (X->n && !sigma_ok(c, X)) return fail(c, PVAC_EINVAL, "compact_plan: X carries no sigma of m_bits");
    C->n = X->n;
    return compact_classify(c, X, C, true, plan);
}

int pvac_hip_compact_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* X, pvac_ct_batch* C) {
    if (!c || !plan || plan->kind != 5 || !batch_ok(X) || !batch_ok(C))
        return fail(c, PVAC_EINVAL, "compact_exec: bad arguments");
    if (X->n != plan->n_pairs || C->n != plan->n_pairs) return fail(c, PVAC_EINVAL, "compact_exec: plan mismatch");
    if (!X->n) return PVAC_OK;
    if (!sigma_ok(c, X) || !sigma_ok(c, C)) return fail(c, PVAC_EINVAL, "compact_exec: X and C must carry sigma of m_bits");
    if (!C->layers || !C->meta || !C->w_lo || !C->w_hi || C->meta == X->meta || C->sigma == X->sigma ||
        C->layers == X->layers)
        return fail(c, PVAC_EINVAL, "compact_exec: C needs row arrays of its own");
    return compact_execute(c, plan, X, C);
}

int pvac_hip_compact_path_count(pvac_hip_ctx* c, uint64_t out[2]) {
    if (!c || !out) return PVAC_EINVAL;
    out[0] = c->compact_path[0];
    out[1] = c->compact_path[1];
    return PVAC_OK;
}

int pvac_hip_ct_recrypt_plan(pvac_hip_ctx* c, const pvac_ct_batch* X, const pvac_ct_batch* pool, pvac_ct_batch* C,
                             pvac_hip_plan* plan) {
    if (!c || !plan || !batch_ok(X) || !batch_ok(pool) || !C || (X->n && (!C->l_off || !C->e_off)))
        return fail(c, PVAC_EINVAL, "ct_recrypt_plan: bad arguments");
    std::memset(plan, 0, sizeof *plan);
    plan->kind = 4;
    plan->n_pairs = X->n;
    C->n = X->n;
    if (!X->n) return PVAC_OK;
    try {
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
            e = launch_exclusive_scan2_u64(C->l_off, C->e_off, X->n, c->scan_scratch.get(), &c->totals[0], &c->totals[1],
                                           c->stream);
        unsigned long long tot[2] = {0, 0};
        if (e == hipSuccess) e = read_back(c, tot, c->totals, sizeof tot);
        if (e != hipSuccess) return hip_fail(c, e, "ct_recrypt_plan");
        plan->total_layer_slots = tot[0];
        plan->total_edge_slots = tot[1];
        plan->max_layers = (uint32_t)std::min<uint64_t>(max_pl, 0xFFFFFFFFu);
        plan->max_nb = (uint32_t)std::min<uint64_t>(max_pe, 0xFFFFFFFFu);
        return PVAC_OK;
    } catch (const std::exception& ex) {
        return fail(c, PVAC_ENOMEM, std::string("ct_recrypt_plan: ") + ex.what());
    }
}

int pvac_hip_ct_recrypt_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* X, const pvac_ct_batch* pool,
                             const uint64_t* picks, pvac_ct_batch* C, uint32_t* iters) {
    if (!c || !plan || plan->kind != 4 || !batch_ok(X) || !batch_ok(pool) || !batch_ok(C))
        return fail(c, PVAC_EINVAL, "ct_recrypt_exec: bad arguments");
    const uint64_t n = X->n, pn = pool->n;
    if (n != plan->n_pairs || C->n != n) return fail(c, PVAC_EINVAL, "ct_recrypt_exec: plan mismatch");
    if (!n) return PVAC_OK;
    if (!c->have_ubk) return fail(c, PVAC_EINVAL, "ct_recrypt_exec: set_ubk first");
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
    try {
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
        if (e == hipSuccess) e = c->rc_idx.grow(17 * n, 17 * std::max<uint64_t>(n, 64));
        if (e == hipSuccess) e = c->rc_ids.grow(n, std::max<uint64_t>(n, 64));
        if (e != hipSuccess) return hip_fail(c, e, "ct_recrypt_exec (shapes)");
        uint64_t* const R = c->rc_idx.get();
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
            e = upload_words(c, c->rc_ids.get(), ids.data(), ids.size() * 4);
            if (e == hipSuccess) e = launch_recrypt_copy(*X, *C, c->rc_ids.get(), ids.size(), m_bits, c->stream);
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
                if (e == hipSuccess) e = upload_words(c, c->rc_ids.get(), fid.data(), f * 4);
                if (e != hipSuccess) return hip_fail(c, e, "ct_recrypt_exec (compact views)");
                const pvac_ct_batch Xs = view_of(base, f, 0);
                pvac_ct_batch Cs = view_of(*C, f, 12);
                pvac_hip_plan cp;
                int rc = compact_classify(c, &Xs, &Cs, false, &cp);
                if (!rc) rc = compact_execute(c, &cp, &Xs, &Cs);
                if (rc) return rc;
                e = launch_scatter_counts(region(13), region(15), c->rc_ids.get(), f, C->l_cnt, C->e_cnt, c->stream);
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
            auto& buf = c->rc_buf[it & 1];
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
            rc = pvac_hip_ct_add_exec(c, &ap, &Av, &Bv, 0, &Cv);
            if (rc) return rc;
            e = launch_ubk_apply(Cv, c->ubk_perm.get(), m_bits, nullptr, c->num_cus, c->stream);
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
    } catch (const std::exception& ex) {
        return fail(c, PVAC_ENOMEM, std::string("ct_recrypt_exec: ") + ex.what());
    }
}

// ---------------------------------------------------------------- LPN PRF
int pvac_hip_ctx_set_secret(pvac_hip_ctx* c, const uint64_t prf_k[4], const uint64_t* lpn_s_host, uint32_t lpn_n,
                            uint32_t lpn_t, uint32_t tau_num, uint32_t tau_den) {
    if (!c || !prf_k || !lpn_s_host) return fail(c, PVAC_EINVAL, "set_secret: arguments");
    const uint32_t words = (lpn_n + 63) / 64;
    if (lpn_n == 0 || words > 64 || tau_den == 0 || tau_num > tau_den)
        return fail(c, PVAC_EINVAL, "set_secret: lpn_n must be in [1, 4096], 0 <= tau_num <= tau_den, tau_den > 0");
    if (lpn_t < 127) return fail(c, PVAC_ENOSYS, "set_secret: lpn_t < 127 not supported");
    c->lpn_s.release();
    c->have_secret = false;
    hipError_t e = c->lpn_s.grow(64, 64);
    if (e == hipSuccess) e = hipMemset(c->lpn_s.get(), 0, 64 * 8);
    if (e == hipSuccess) e = hipMemcpy(c->lpn_s.get(), lpn_s_host, (size_t)words * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(c, e, "set_secret");
    std::memcpy(c->prf_k, prf_k, 32);
    c->lpn_words = words;
    c->lpn_t = lpn_t;
    c->tau_num = tau_num;
    c->tau_den = tau_den;
    c->have_secret = true;
    return PVAC_OK;
}

int pvac_hip_ctx_set_H_digest(pvac_hip_ctx* c, const uint8_t digest[32]) {
    if (!c || !digest) return PVAC_EINVAL;
    std::memcpy(c->H_digest, digest, 32);
    c->have_digest = true;
    return PVAC_OK;
}

namespace {

uint64_t fnv1a(const char* d) {   // lpn.hpp:150-157
    uint64_t h = 0xcbf29ce484222325ull;
    for (const char* p = d; *p; ++p) { h ^= (uint8_t)*p; h *= 0x100000001b3ull; }
    return h;
}

// constants of the key derivation (lpn.hpp:159-186); the first message block is fixed per key
int prf_setup(pvac_hip_ctx* c, prf_consts& k) {
    if (!c->have_secret) return fail(c, PVAC_EINVAL, "prf: secret key not set (pvac_hip_ctx_set_secret)");
    if (!c->have_digest) return fail(c, PVAC_EINVAL, "prf: H_digest unknown (gen_H, set_H or set_H_digest)");
    if (!c->aes_tables) {
        hipError_t e = prf_upload_tables(c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "prf tables");
        c->aes_tables = true;
    }
    uint8_t m[64];
    for (int i = 0; i < 4; ++i)
        for (int b = 0; b < 8; ++b) m[8 * i + b] = (uint8_t)(c->prf_k[i] >> (8 * b));
    for (int b = 0; b < 8; ++b) m[32 + b] = (uint8_t)(c->prm.canon_tag >> (8 * b));
    std::memcpy(m + 40, c->H_digest, 24);
    uint32_t w[16];
    for (int i = 0; i < 16; ++i)
        w[i] = (uint32_t)m[4 * i] << 24 | (uint32_t)m[4 * i + 1] << 16 | (uint32_t)m[4 * i + 2] << 8 | m[4 * i + 3];
    sha_state st;
    sha_init(st);
    sha_compress(st, w);
    std::memcpy(k.mid, st.h, 32);
    uint64_t tail = 0;
    for (int b = 0; b < 8; ++b) tail |= (uint64_t)c->H_digest[24 + b] << (8 * b);
    k.hd_tail = tail;
    static const char* const doms[6] = {"pvac.prf.r.1", "pvac.prf.r.2", "pvac.prf.r.3",
                                        "pvac.prf.noise.1", "pvac.prf.noise.2", "pvac.prf.noise.3"};
    for (int d = 0; d < 6; ++d) k.dom_hash[d] = fnv1a(doms[d]);
    k.toep_hash = fnv1a("pvac.dom.toeplitz");
    k.s_bits = c->lpn_s.get();
    k.s_words = c->lpn_words;
    k.tau_num = c->tau_num;
    k.tau_den = c->tau_den;
    return PVAC_OK;
}

int ensure_prf_scratch(pvac_hip_ctx* c, uint64_t cores) {
    int rc = hip_fail(c, c->prf_req.grow_floor(cores * prf_request_bytes()), "alloc prf requests");
    if (rc) return rc;
    return hip_fail(c, c->prf_core.grow_floor(2 * cores), "alloc prf cores");
}

}  // namespace

int pvac_hip_prf(pvac_hip_ctx* c, int kind, size_t n, const uint64_t* seeds, uint64_t* out) {
    if (!c || kind < 0 || kind > 7 || (n && (!seeds || !out))) return fail(c, PVAC_EINVAL, "prf: arguments");
    if (!n) return PVAC_OK;
    prf_consts k{};
    int rc = prf_setup(c, k);
    if (rc) return rc;
    rc = ensure_prf_scratch(c, 3 * (uint64_t)n);
    if (rc) return rc;
    scoped_timer t(c, "prf");
    return hip_fail(c, launch_prf(k, kind, seeds, n, c->prf_req.get(), c->prf_core.get(), out, c->stream), "prf");
}

// ---------------------------------------------------------------- enc_value
namespace {
// ops/encrypt.hpp:16-27 with the context's noise Params (the reference's defaults: noise_entropy_bits
// 120, tuple2_fraction 0.55, depth_slope_bits 16; pvac_hip_ctx_set_noise); enc_value uses depth_hint 0
void plan_noise(const pvac_hip_ctx* c, int depth, uint32_t& z2, uint32_t& z3) {
    const uint32_t B = c->prm.B;
    const double budget = c->noise_bits + c->noise_slope * std::max(0, depth);
    const double per2 = 2.0 * std::log2((double)B), per3 = 3.0 * std::log2((double)B);
    int a = std::max(0, (int)std::floor((budget * c->noise_t2) / std::max(1e-6, per2)));
    int b = std::max(0, (int)std::floor((budget * (1.0 - c->noise_t2)) / std::max(1e-6, per3)));
    if (a + b == 1) { if (b > 0) ++b; else ++a; }
    z2 = (uint32_t)a;
    z3 = (uint32_t)b;
}
}  // namespace

int pvac_hip_enc_caps(pvac_hip_ctx* c, uint32_t* layers_per_value, uint32_t* edges_per_value, uint32_t* draws_hint) {
    return pvac_hip_enc_caps_depth(c, 0, layers_per_value, edges_per_value, draws_hint);
}

int pvac_hip_enc_caps_depth(pvac_hip_ctx* c, int depth_hint, uint32_t* layers_per_value, uint32_t* edges_per_value,
                            uint32_t* draws_hint) {
    if (!c) return PVAC_EINVAL;
    uint32_t z2, z3;
    plan_noise(c, depth_hint, z2, z3);
    if ((uint64_t)8 + 2ull * z2 + 3ull * z3 > kEncPreMax)
        return fail(c, PVAC_ENOSYS, "enc_caps: noise plan beyond 256 pre-merge edges per half (depth hint > 124 with the default Params)");
    const uint32_t npre = 8 + 2 * z2 + 3 * z3;
    if (layers_per_value) *layers_per_value = 2;
    if (edges_per_value) *edges_per_value = 2 * npre;
    // mask 2 + per half: nonce 2, signal 2*8 + 2*7, salts npre, noise picks/signs/coefficients, shuffle
    if (draws_hint) *draws_hint = 2 + 2 * (2 + 16 + 14 + npre + z2 * 5 + z3 * 10 + npre) + 64;
    return PVAC_OK;
}

int pvac_hip_enc_value(pvac_hip_ctx* c, size_t n, const uint64_t* values, const uint64_t* rnd, uint32_t rnd_stride,
                       pvac_ct_batch* C, uint32_t flags, uint32_t* status) {
    return pvac_hip_enc_value_depth(c, n, values, rnd, rnd_stride, 0, C, flags, status);
}

int pvac_hip_enc_value_depth(pvac_hip_ctx* c, size_t n, const uint64_t* values, const uint64_t* rnd, uint32_t rnd_stride,
                             int depth_hint, pvac_ct_batch* C, uint32_t flags, uint32_t* status) {
    if (!c || !C || (n && (!values || !rnd || !status))) return fail(c, PVAC_EINVAL, "enc_value: arguments");
    if (!C->l_off || !C->l_cnt || !C->layers || !C->e_off || !C->e_cnt || !C->meta || !C->w_lo || !C->w_hi)
        return fail(c, PVAC_EINVAL, "enc_value: output arrays");
    const bool with_sigma = (flags & PVAC_ENC_WITH_SIGMA) != 0;
    if (with_sigma && (!C->sigma || !c->H.ready || C->sigma_words != c->prm.m_bits / 64))
        return fail(c, PVAC_EINVAL, "enc_value: WITH_SIGMA needs C->sigma (m_bits/64 words per edge) and H");
    if (!c->powg.get()) return fail(c, PVAC_EINVAL, "enc_value: powg_B not set (pvac_hip_ctx_set_powg)");
    C->n = n;
    if (!n) return PVAC_OK;
    prf_consts k{};
    int rc = prf_setup(c, k);
    if (rc) return rc;
    enc_plan_args a{};
    a.values = values;
    a.rnd = rnd;
    a.stride = rnd_stride;
    a.B = c->prm.B;
    plan_noise(c, depth_hint, a.Z2, a.Z3);
    a.n = n;
    a.canon = c->prm.canon_tag;
    a.powg = c->powg.get();
    const uint32_t npre = 8 + 2 * a.Z2 + 3 * a.Z3;
    if ((uint64_t)8 + 2ull * a.Z2 + 3ull * a.Z3 > kEncPreMax)
        return fail(c, PVAC_ENOSYS, "enc_value: noise plan beyond 256 pre-merge edges per half (depth hint > 124 with the default Params)");
    const uint64_t cores = (uint64_t)n * enc_cores_per_value(a.Z2, a.Z3);
    const uint64_t pe = (uint64_t)n * 2 * npre;
    const uint32_t sw = c->prm.m_bits / 64;
    // arena: halves | requests | cores | pre CSR (4 x n) | pre layers | meta, w_lo, w_hi, salt | sigma
    auto al = [](uint64_t b) { return (b + 255) & ~255ull; };
    const uint64_t off_req = al((uint64_t)2 * n * enc_half_bytes(npre));
    const uint64_t off_core = off_req + al(cores * prf_request_bytes());
    const uint64_t off_csr = off_core + al(cores * 16);
    const uint64_t off_lay = off_csr + al((uint64_t)n * 32);
    const uint64_t off_e = off_lay + al((uint64_t)n * 2 * sizeof(pvac_layer));
    const uint64_t off_sig = off_e + al(pe * 32);
    const uint64_t total = off_sig + (with_sigma ? al(pe * sw * 8) : 0);
    if (const hipError_t ea = c->enc_arena.grow(total, total)) return hip_fail(c, ea, "alloc enc scratch");
    uint8_t* A = c->enc_arena.get();
    pvac_ct_batch pre{};
    pre.n = n;
    pre.l_off = (uint64_t*)(A + off_csr);
    pre.l_cnt = pre.l_off + n;
    pre.e_off = pre.l_cnt + n;
    pre.e_cnt = pre.e_off + n;
    pre.layers = (pvac_layer*)(A + off_lay);
    pre.meta = (uint64_t*)(A + off_e);
    pre.w_lo = pre.meta + pe;
    pre.w_hi = pre.w_lo + pe;
    uint64_t* pre_salt = pre.w_hi + pe;
    pre.sigma = with_sigma ? (uint64_t*)(A + off_sig) : nullptr;
    pre.sigma_words = with_sigma ? sw : 0;
    scoped_timer t(c, "enc_value");
    hipError_t e = launch_enc_plan(a, A, (prf_request*)(A + off_req), pre, pre_salt, status, c->stream);
    if (e == hipSuccess) e = launch_prf_cores(k, A + off_req, cores, (uint64_t*)(A + off_core), c->stream);
    if (e == hipSuccess) e = launch_enc_weights(a, A, (const uint64_t*)(A + off_core), pre, c->stream);
    if (e == hipSuccess && with_sigma) e = launch_sigma(c->H, c->prm, pre, pre_salt, nullptr, c->num_cus, c->stream);
    pvac_ct_batch out = *C;
    if (!with_sigma) out.sigma = nullptr;
    if (e == hipSuccess) e = launch_enc_finish(a, A, pre, out, status, c->stream);
    return hip_fail(c, e, "enc_value");
}

int pvac_hip_base_R(pvac_hip_ctx* c, const pvac_ct_batch* X, uint64_t* R_out) {
    if (!c || !batch_ok(X) || (X->n && !R_out)) return fail(c, PVAC_EINVAL, "base_R: arguments");
    if (!X->n) return PVAC_OK;
    prf_consts k{};
    int rc = prf_setup(c, k);
    if (rc) return rc;
    // layer slots are addressed through l_off / l_cnt on the device: gather every slot's seed
    std::vector<uint64_t> lo(X->n), lc(X->n);
    hipError_t e = hipMemcpyAsync(lo.data(), X->l_off, X->n * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(lc.data(), X->l_cnt, X->n * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "base_R (offsets)");
    uint64_t slots = 0;
    for (uint64_t i = 0; i < X->n; ++i) slots = std::max(slots, lo[i] + lc[i]);
    if (!slots) return PVAC_OK;
    rc = ensure_prf_scratch(c, 4 * slots);   // 3 cores per slot + the BASE flags behind them
    if (rc) return rc;
    scoped_timer t(c, "base_R");
    return hip_fail(c, launch_base_R(k, *X, slots, c->prf_req.get(), c->prf_core.get(), R_out, c->stream), "base_R");
}

// ---------------------------------------------------------------- measured ALU ceilings
int pvac_hip_alu_ceiling(pvac_hip_ctx* c, int kind, double* per_s) {
    if (!c || !per_s || kind < 0 || kind > 5) return fail(c, PVAC_EINVAL, "alu_ceiling: bad arguments");
    const hipError_t e = run_alu_probe(kind, c->num_cus, c->stream, per_s);
    return e == hipSuccess ? PVAC_OK : hip_fail(c, e, "alu_ceiling");
}

int pvac_hip_issue_probe(pvac_hip_ctx* c, int op, int waves_per_simd, double* per_s, double* clock_hz) {
    if (!c || !per_s || !clock_hz) return fail(c, PVAC_EINVAL, "issue_probe: bad arguments");
    const hipError_t e = run_issue_probe(op, waves_per_simd, c->num_cus, c->stream, per_s, clock_hz);
    return e == hipSuccess ? PVAC_OK : hip_fail(c, e, "issue_probe");
}

// ---------------------------------------------------------------- gsum invariant
int pvac_hip_check_mul_gsum(pvac_hip_ctx* c, const pvac_ct_batch* A, const pvac_ct_batch* B, const pvac_ct_batch* C,
                            const uint64_t* nonces, uint32_t* status, uint64_t* n_bad) {
    if (!c || !n_bad || !batch_ok(A) || !batch_ok(B) || !batch_ok(C) || !nonces)
        return fail(c, PVAC_EINVAL, "check_mul_gsum: bad arguments");
    if (A->n != B->n || A->n != C->n) return fail(c, PVAC_EINVAL, "check_mul_gsum: batch sizes differ");
    if (!c->powg.get()) return fail(c, PVAC_EINVAL, "check_mul_gsum: powg_B not set (pvac_hip_ctx_set_powg)");
    *n_bad = 0;
    if (!A->n) return PVAC_OK;
    hipError_t e = c->check_buf.grow(8, 8);
    if (e == hipSuccess) e = hipMemsetAsync(c->check_buf.get(), 0, 32, c->stream);
    if (e == hipSuccess) e = launch_check_sizes(*A, *B, *C, c->check_buf.get(), c->stream);
    unsigned int mx[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(mx, c->check_buf.get(), sizeof mx, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "check_mul_gsum (sizes)");
    unsigned long long* cnt = (unsigned long long*)(c->check_buf.get() + 4);
    // layer tables beyond one workgroup's LDS (chain depth 9 on): per-workgroup slabs in global memory
    const uint64_t gs = check_gsum_scratch_bytes(c->prm.B, mx, A->n, c->num_cus);
    if (gs) {
        const int rc = hip_fail(c, c->check_scratch.grow_floor((size_t)gs), "alloc gsum check scratch");
        if (rc) return rc;
    }
    e = launch_check_gsum(*A, *B, *C, nonces, c->powg.get(), c->prm.B, mx, status, cnt, c->num_cus, gs ? c->check_scratch.get() : nullptr,
                          c->stream);
    if (e == hipErrorInvalidValue) return fail(c, PVAC_ERANGE, "check_mul_gsum: no scratch for the layer tables");
    unsigned long long bad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, cnt, sizeof bad, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "check_mul_gsum");
    c->check_path[gs ? 1 : 0]++;
    *n_bad = bad;
    return PVAC_OK;
}

int pvac_hip_check_mul_gsum_path_count(pvac_hip_ctx* c, uint64_t out[2]) {
    if (!c || !out) return PVAC_EINVAL;
    out[0] = c->check_path[0];
    out[1] = c->check_path[1];
    return PVAC_OK;
}

// ---------------------------------------------------------------- dec_value
int pvac_hip_ctx_set_powg(pvac_hip_ctx* c, const uint64_t* powg_host, uint32_t count) {
    if (!c || !powg_host || count < c->prm.B) return fail(c, PVAC_EINVAL, "set_powg: need B (lo, hi) pairs");
    c->powg.release();
    c->powg_n = 0;
    hipError_t e = c->powg.grow(2 * (size_t)count, 2 * (size_t)count);
    if (e == hipSuccess) e = hipMemcpy(c->powg.get(), powg_host, (size_t)count * 16, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(c, e, "set_powg");
    c->powg_n = count;
    return PVAC_OK;
}

int pvac_hip_dec_value(pvac_hip_ctx* c, const pvac_ct_batch* X, const uint64_t* R_base, uint64_t* out,
                       uint32_t* status) {
    if (!c || !batch_ok(X) || !out || !status || (X->n && !R_base)) return fail(c, PVAC_EINVAL, "dec_value: arguments");
    if (!c->powg.get()) return fail(c, PVAC_EINVAL, "dec_value: powg_B not set (pvac_hip_ctx_set_powg)");
    if (!X->n) return PVAC_OK;
    int rc = ensure_pairs(c, X->n);
    if (rc) return rc;
    rc = hip_fail(c, c->dec_roff.grow_floor(X->n), "alloc dec offsets");
    if (rc) return rc;
    // dense per-cipher layer offsets (the batch may be capacity-padded)
    hipError_t e = hipMemcpyAsync(c->dec_roff.get(), X->l_cnt, X->n * 8, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = launch_exclusive_scan_u64(c->dec_roff.get(), X->n, c->scan_scratch.get(), &c->totals[0], c->stream);
    unsigned long long total = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&total, &c->totals[0], 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "dec_value (offsets)");
    const size_t need = dec_scratch_bytes(total);
    e = c->dec_scratch.grow(need, need);
    if (e != hipSuccess) return hip_fail(c, e, "alloc dec scratch");
    scoped_timer t(c, "dec_value");
    return hip_fail(c,
                    launch_dec_value(*X, R_base, c->powg.get(), c->prm.B, c->dec_roff.get(), total, c->dec_scratch.get(), out, status,
                                     c->stream),
                    "dec_value");
}

// ---------------------------------------------------------------- synthetic / checks
int pvac_hip_gen_fresh_batch(pvac_hip_ctx* c, uint64_t seed, uint32_t epl, pvac_ct_batch* X) {
    return pvac_hip_gen_fresh_batch_at(c, seed, 0, epl, X);
}

int pvac_hip_gen_fresh_batch_at(pvac_hip_ctx* c, uint64_t seed, uint64_t first_index, uint32_t epl,
                                pvac_ct_batch* X) {
    if (!c || !batch_ok(X) || !X->layers || !X->meta || !X->w_lo || !X->w_hi) return PVAC_EINVAL;
    return hip_fail(c, launch_gen_fresh(seed, first_index, epl, c->prm.B, *X, c->stream), "gen_fresh");
}

int pvac_hip_fill_nonces(pvac_hip_ctx* c, uint64_t seed, uint64_t first_index, const pvac_ct_batch* A,
                         const pvac_ct_batch* B, const pvac_ct_batch* C, uint64_t* out) {
    if (!c || !batch_ok(A) || !batch_ok(B) || !C || !C->l_off || (A->n && !out) || A->n != B->n) return PVAC_EINVAL;
    return hip_fail(c, launch_fill_nonces(seed, first_index, *A, *B, C->l_off, out, c->stream), "fill_nonces");
}

int pvac_hip_fill_random(pvac_hip_ctx* c, uint64_t seed, uint64_t* out, size_t n) {
    if (!c || (n && !out)) return PVAC_EINVAL;
    return hip_fail(c, launch_fill_random(seed, out, n, c->stream), "fill_random");
}

uint64_t pvac_hip_bucket_count(uint64_t n) { return bucket_count_after_reserve(n); }

int pvac_hip_batch_digest(pvac_hip_ctx* c, const pvac_ct_batch* X, uint64_t* out) {
    if (!c || !batch_ok(X) || (X->n && !out)) return PVAC_EINVAL;
    return hip_fail(c, launch_batch_digest(*X, out, c->stream), "batch_digest");
}

int pvac_hip_commit_ct(pvac_hip_ctx* c, const pvac_ct_batch* X, uint8_t* digests) {
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
}

int pvac_hip_batch_sumdigest(pvac_hip_ctx* c, const pvac_ct_batch* X, uint64_t* out) {
    if (!c || !batch_ok(X) || (X->n && !out)) return PVAC_EINVAL;
    return hip_fail(c, launch_batch_sumdigest(*X, out, c->stream), "batch_sumdigest");
}

// The used rows of a capacity-padded batch packed back to back (a plan's output keeps every pair's
// capacity): dst's counts = src's, its offsets their exclusive scans, rows (and sigma when both
// carry it) copied by k_stage_rows. totals[0], [1] = the packed layer / edge counts, so a caller
// copies exactly those rows to the host. dst's row arrays must hold the packed rows (src's
// capacity always does); the pair scratch of a pending plan is left alone.
int pvac_hip_batch_pack(pvac_hip_ctx* c, const pvac_ct_batch* src, pvac_ct_batch* dst, uint64_t* totals) {
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
        e = launch_exclusive_scan2_u64(dst->l_off, dst->e_off, n, c->scan_scratch.get(), &c->totals[0], &c->totals[1],
                                       c->stream);
    unsigned long long tot[2] = {0, 0};
    if (e == hipSuccess) e = read_back(c, tot, c->totals, sizeof tot);
    if (e != hipSuccess) return hip_fail(c, e, "batch_pack (offsets)");
    totals[0] = tot[0];
    totals[1] = tot[1];
    return hip_fail(c, launch_stage_rows(*src, *dst, c->stream), "batch_pack (rows)");
}

// ---------------------------------------------------------------- depth chains
}  // extern "C"

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
    void failed(int code, const std::string& msg) {
        std::lock_guard<std::mutex> g(mu);
        if (rc == PVAC_OK) {
            rc = code;
            err = msg;
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
    if (ensure_pairs(k, kk)) {
        sh->failed(PVAC_ENOMEM, "ct_mul_chain: stage scratch: " + k->err);
        return false;
    }
    const int sd = sh->x_dev, dd = k->device;
    if (!chain_ok(sh, hipMemcpyPeerAsync(S.l_cnt.get(), dd, src.l_cnt, sd, kk * 8, k->stream), "stage counts") ||
        !chain_ok(sh, hipMemcpyPeerAsync(S.e_cnt.get(), dd, src.e_cnt, sd, kk * 8, k->stream), "stage counts") ||
        !chain_ok(sh, hipMemcpyAsync(S.l_off.get(), S.l_cnt.get(), kk * 8, hipMemcpyDeviceToDevice, k->stream), "stage offsets") ||
        !chain_ok(sh, hipMemcpyAsync(S.e_off.get(), S.e_cnt.get(), kk * 8, hipMemcpyDeviceToDevice, k->stream), "stage offsets") ||
        !chain_ok(sh, launch_exclusive_scan_u64(S.l_off.get(), kk, k->scan_scratch.get(), &k->totals[0], k->stream), "stage scan") ||
        !chain_ok(sh, launch_exclusive_scan_u64(S.e_off.get(), kk, k->scan_scratch.get(), &k->totals[1], k->stream), "stage scan"))
        return false;
    unsigned long long tot[2] = {0, 0};
    if (!chain_ok(sh, hipMemcpyAsync(tot, k->totals, sizeof tot, hipMemcpyDeviceToHost, k->stream), "stage totals") ||
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
    if (!chain_ok(sh, k->chain_salts.grow_headroom(slots, k->stream), "sigma alloc salts")) return false;
    if (o.salts_at) {
        if (o.salts_at(o.user, d, c0, &A, &Xv, &C, k->chain_salts.get(), plan.total_edge_slots, (void*)k->stream) != 0) {
            sh->failed(PVAC_EINVAL, "ct_mul_chain: salts_at callback failed");
            return false;
        }
    } else if (!chain_ok(sh,
                         launch_fill_random(o.nonce_seed ^ 0x5A175A175A175A17ull ^ (97ull * c0 + d), k->chain_salts.get(), slots,
                                            k->stream),
                         "sigma fill salts")) {
        return false;
    }
    C.sigma = S.sigma.get();
    C.sigma_words = sw;
    bool hash_order = (mflags & PVAC_MUL_ORDER_CANONICAL) == 0;
    if (hash_order) {
        std::vector<uint32_t> stv(C.n);
        if (!chain_ok(sh, hipMemcpyAsync(stv.data(), k->pair_status.get(), C.n * 4, hipMemcpyDeviceToHost, k->stream), "sigma status") ||
            !chain_ok(sh, hipStreamSynchronize(k->stream), "sigma status"))
            return false;
        for (uint32_t v : stv) hash_order &= v != 1u;
    }
    if (hash_order) return chain_ok(sh, launch_sigma(k->H, k->prm, C, k->chain_salts.get(), nullptr, k->num_cus, k->stream), "sigma launch");
    if (ct_mul_exec(k, &plan, &A, &Xv, k->chain_nonces.get(), k->chain_salts.get(), &C, mflags | PVAC_MUL_WITH_SIGMA,
                    {a_img, nullptr, nullptr})) {
        sh->failed(PVAC_EDEVICE, "ct_mul_chain: sigma exec: " + k->err);
        return false;
    }
    return true;
}

// one worker: chunks of its device range in input order from the range's counter, depth steps of
// plan + exec each on this context's stream, the final c_depth to the digests / on_chunk
void chain_worker(pvac_hip_ctx* k, chain_shared* sh, chain_range* rg, bool stage, chain_wstats* ws) {
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
        if ((stage || remote) && !stage_chunk(k, sh, chain_view(X, c0, kk), Xv, k->chain_stage)) return;
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
                if ((stage || remote) && !stage_chunk(k, sh, chain_view(o.operands[d], c0, kk), Xv, k->chain_stage_op))
                    return;
            }
            chain_set& S = k->chain_bufs[cur];
            if (!chain_ok(sh, S.grow_index(kk, k->stream), "alloc offsets / counts")) return;
            pvac_ct_batch C = S.view(kk);   // the plan writes its offsets and counts; the rows are sized below
            pvac_hip_plan plan{};
            if (!rcchk(pvac_hip_ct_mul_plan(k, &A, &Xv, &C, &plan), "plan")) return;
            // an output array that does not fit first takes this worker's scratch arena back (the
            // general path reallocates it within what is left, splitting its sub-batch if needed)
            auto grow_out = [&](auto& b, size_t need, const char* what) -> bool {
                hipError_t e = b.grow_headroom(need, k->stream);
                if (e == hipErrorOutOfMemory && k->arena.get()) {
                    (void)hipGetLastError();
                    e = hipStreamSynchronize(k->stream);
                    k->arena.release();
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
            if (!chain_ok(sh, k->chain_nonces.grow_headroom(nw, k->stream), "alloc nonces")) return;
            C = S.view(kk);
            if (o.nonces_at) {
                if (o.nonces_at(o.user, d, c0, &A, &Xv, &C, k->chain_nonces.get(), nw, (void*)k->stream) != 0) {
                    sh->failed(PVAC_EINVAL, "ct_mul_chain: nonces_at callback failed");
                    return;
                }
            } else if (o.fill_nonces) {
                if (o.fill_nonces(o.user, d, c0, nw, k->chain_nonces.get(), (void*)k->stream) != 0) {
                    sh->failed(PVAC_EINVAL, "ct_mul_chain: fill_nonces callback failed");
                    return;
                }
            } else if (!chain_ok(sh, launch_fill_random(o.nonce_seed + 97ull * c0 + d, k->chain_nonces.get(), nw, k->stream),
                               "fill nonces")) {
                return;
            }
            uint32_t* c_img = nullptr;
            if (use_img && d + 1 < o.depth) {
                if (!chain_ok(sh, S.img.grow_headroom(kk, k->stream), "alloc image flags")) return;
                if (!chain_ok(sh, hipMemsetAsync(S.img.get(), 0, kk * 4, k->stream), "image flags")) return;
                c_img = S.img.get();
            }
            const step_images img{a_img, c_img, k->chain_stats.get() + 2 * PVAC_CHAIN_MAX_DEPTH};
            if (!rcchk(ct_mul_exec(k, &plan, &A, &Xv, k->chain_nonces.get(), nullptr, &C, mflags, img), "exec")) return;
            if (!chain_ok(sh, launch_chain_stats(A, Xv, C, k->chain_stats.get() + 2 * d, k->stream), "stats")) return;
            if (check) {
                uint64_t bad = 0;
                if (!rcchk(pvac_hip_check_mul_gsum(k, &A, &Xv, &C, k->chain_nonces.get(), nullptr, &bad), "gsum check"))
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
            if (!chain_ok(sh, k->chain_out.grow_headroom(m, k->stream), "alloc outputs") || !put(k->chain_out.get()))
                return false;
            return chain_ok(sh, hipMemcpyPeerAsync(dst + c0, sh->x_dev, k->chain_out.get(), k->device, m * 8, k->stream), "peer copy");
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

}  // namespace

extern "C" {

int pvac_hip_memcpy(void* dst, const void* src, size_t bytes, void* stream) {
    if (!bytes) return PVAC_OK;
    if (!dst || !src) return PVAC_EINVAL;
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? PVAC_OK : PVAC_EDEVICE;
}

int pvac_hip_chain_partition(uint64_t n, uint64_t chunk, uint32_t parts, uint64_t* first) {
    if (!first || parts == 0 || parts > PVAC_CHAIN_MAX_DEVICES) return PVAC_EINVAL;
    if (!chunk) chunk = 1024;
    const uint64_t nch = (n + chunk - 1) / chunk;   // whole chunks, dealt as evenly as possible
    for (uint32_t j = 0; j <= parts; ++j) first[j] = std::min<uint64_t>(n, (nch * j / parts) * chunk);
    return PVAC_OK;
}

int pvac_hip_ct_mul_chain(pvac_hip_ctx* c, const pvac_ct_batch* X, const pvac_chain_opts* o, pvac_chain_stats* st) {
    if (!c || !o || !st || !batch_ok(X)) return fail(c, PVAC_EINVAL, "ct_mul_chain: bad arguments");
    if (o->depth < 1 || o->depth > PVAC_CHAIN_MAX_DEPTH) return fail(c, PVAC_EINVAL, "ct_mul_chain: depth");
    if (o->flags & ~(PVAC_MUL_ORDER_CANONICAL | PVAC_CHAIN_CHECK_GSUM | PVAC_MUL_WITH_SIGMA | PVAC_CHAIN_STAGE_INPUTS |
                     PVAC_CHAIN_IMG_BATCH2))
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
    if (!c->chain_kids.empty() && layout != c->chain_layout) {
        for (pvac_hip_ctx* k : c->chain_kids) {
            hipSetDevice(k->device);
            e = release_chain_worker(k);
            if (e != hipSuccess) return hip_fail(c, e, "ct_mul_chain: worker release");
        }
    }
    c->chain_layout = layout;
    // worker contexts: [range j * S + w] on devs[j]; a layout change rebuilds the ones that differ
    if (c->chain_kids.size() > (size_t)D * S) {
        for (size_t w = (size_t)D * S; w < c->chain_kids.size(); ++w) pvac_hip_ctx_destroy(c->chain_kids[w]);
        c->chain_kids.resize((size_t)D * S);
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
            if (slot < c->chain_kids.size() && c->chain_kids[slot]->device != devs[j]) {
                pvac_hip_ctx_destroy(c->chain_kids[slot]);
                c->chain_kids[slot] = nullptr;
            }
            if (slot >= c->chain_kids.size()) c->chain_kids.push_back(nullptr);
            pvac_hip_ctx*& k = c->chain_kids[slot];
            if (!k) {
                const int rc = pvac_hip_ctx_create(devs[j], &c->prm, &k);
                if (rc) return fail(c, rc, "ct_mul_chain: worker context");
            }
            e = k->chain_stats.grow(2 * PVAC_CHAIN_MAX_DEPTH + 1, 2 * PVAC_CHAIN_MAX_DEPTH + 1);
            if (e != hipSuccess) return hip_fail(c, e, "ct_mul_chain: worker statistics");
            k->arena_cap_words = cap_words;
            k->prm = c->prm;
            k->spin_us = 200;
            k->img_grid_y = (o->flags & PVAC_CHAIN_IMG_BATCH2) ? 2u : 65535u;
            if (c->powg.get() && (k->powg_n != c->powg_n || !k->powg.get())) {
                k->powg.release();
                e = k->powg.grow(2 * (size_t)c->powg_n, 2 * (size_t)c->powg_n);
                if (e != hipSuccess) return hip_fail(c, e, "ct_mul_chain: worker powg");
                k->powg_n = c->powg_n;
            }
            e = hipSuccess;
            if (c->powg.get()) e = hipMemcpyPeer(k->powg.get(), k->device, c->powg.get(), c->device, (size_t)c->powg_n * 16);
            if (e == hipSuccess && (o->flags & PVAC_MUL_WITH_SIGMA) && (!k->H.ready || k->H_from != c->H_gen)) {
                e = sigma_tables_clone(k->H, c->H, k->device, c->device, k->stream);
                k->H_from = c->H_gen;
            }
            if (e == hipSuccess) e = hipMemsetAsync(k->chain_stats.get(), 0, (2 * PVAC_CHAIN_MAX_DEPTH + 1) * 8, k->stream);
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
    for (size_t w = 0; w < nk; ++w) redo0[w] = c->chain_kids[w]->redo_total;
    std::vector<std::thread> th;
    th.reserve(nk);
    for (uint32_t j = 0; j < D; ++j)
        for (uint32_t w = 0; w < S; ++w)
            th.emplace_back(chain_worker, c->chain_kids[(size_t)j * S + w], &sh, &ranges[j],
                            j > 0 && (o->flags & PVAC_CHAIN_STAGE_INPUTS) != 0, &ws[(size_t)j * S + w]);
    for (std::thread& t : th) t.join();
    for (size_t w = 0; w < nk; ++w) {
        pvac_hip_ctx* k = c->chain_kids[w];
        hipSetDevice(k->device);
        e = hipStreamSynchronize(k->stream);
        if (e != hipSuccess && sh.rc == PVAC_OK) {
            hip_fail(c, e, "ct_mul_chain");
            sh.failed(PVAC_EDEVICE, c->err);
        }
        unsigned long long v[2 * PVAC_CHAIN_MAX_DEPTH + 1];
        if (hipMemcpy(v, k->chain_stats.get(), sizeof v, hipMemcpyDeviceToHost) == hipSuccess) {
            for (uint32_t d = 0; d < o->depth; ++d) {
                st->edges[d] += v[2 * d];
                st->products[d] += v[2 * d + 1];
            }
            st->image_steps += v[2 * PVAC_CHAIN_MAX_DEPTH];
        }
        st->gsum_pairs += ws[w].gsum_pairs;
        st->gsum_failed += ws[w].gsum_failed;
        st->chunks += ws[w].chunks;
        st->redo += k->redo_total - redo0[w];
    }
    st->pair_steps = X->n * o->depth;
    st->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (sh.rc != PVAC_OK) return fail(c, sh.rc, sh.err);
    return PVAC_OK;
}

}  // extern "C"

