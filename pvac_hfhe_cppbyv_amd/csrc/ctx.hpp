// ctx.hpp — the host runtime's context and what its translation units (rt_*.cpp) share: the
// extern "C" ABI of include/pvac_hip.h is split by operation over those units, and every one of them
// sees the same pvac_hip_ctx, the plan scratch type, the exception boundary and the small helpers
// below. Host code only: no .hip file includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <exception>
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "common.hpp"
#include "dev_mem.hpp"
#include "drbg.hpp"
#include "large_plan.hpp"
#include "sigma.hpp"

namespace pvhip {

constexpr uint32_t kNbTableLen = kFreshProdMax + 1;   // bucket counts for |A.E||B.E| in [0, 4096]

// The per-pair scratch the ct_mul, ct_add and compact plans share, and the rule that keeps an exec
// from reading another plan's classes: only the latest plan may be exec'd. Every plan pass starts
// with begin(), which takes a new stamp whether or not it reallocates, so no growth of the arrays
// can leave an older plan valid; a plan is stamped by commit() only once it has succeeded.
struct plan_scratch {
    dev_buf<uint8_t> pair_class;
    dev_buf<uint32_t> pair_status;
    dev_buf<fresh_rec> fresh_recs;   // per-pair header records of the fresh ct_mul path
    dev_buf<uint64_t> large_ids, large_info;   // 5 (mul) or 8 (merge set) words of large_info per pair
    dev_buf<uint64_t> redo_ids;      // fresh-kernel pairs left to the general path (a key sum of 0)
    dev_buf<unsigned int> redo_cnt;
    bool redo_cnt_dirty = true;      // redo_cnt may be nonzero (zeroed before the next exec)
    dev_buf<plan_stats> stats;
    unsigned long long* totals = nullptr;   // [2]: &stats->total_layers (layer and edge slot totals), not owned

    // the one plan_stats record; the scans' two totals are its first words, so a plan reads stats
    // and totals back in one copy
    hipError_t init() {
        const hipError_t e = stats.grow(1, 1);
        if (e == hipSuccess) totals = &stats.get()->total_layers;
        return e;
    }
    // pairs the six arrays hold (redo_ids is grown last: its capacity stands for all of them)
    size_t capacity() const { return redo_ids.capacity(); }
    // A new plan over n pairs: every earlier plan goes stale, then the arrays grow together. A failed
    // growth gives back all it took and leaves capacity 0.
    hipError_t begin(size_t n) {
        invalidate();
        hipError_t e = redo_cnt.grow(4, 4);
        if (e == hipSuccess && n > capacity()) {
            drop_pairs();
            const size_t cap = std::max<size_t>(n, 1024);
            e = pair_class.grow(n, cap);
            if (e == hipSuccess) e = pair_status.grow(n, cap);
            if (e == hipSuccess) e = large_ids.grow(n, cap);
            if (e == hipSuccess) e = large_info.grow(8 * n, 8 * cap);
            if (e == hipSuccess) e = fresh_recs.grow(n, cap);
            if (e == hipSuccess) e = redo_ids.grow(n, cap);
        }
        if (e != hipSuccess) {
            drop_pairs();
            redo_cnt.release();
            redo_cnt_dirty = true;
        }
        return e;
    }
    void commit(pvac_hip_plan* plan) const { plan->reserved[0] = stamp_; }
    // an uncommitted plan carries 0, which is never a stamp
    bool is_latest(const pvac_hip_plan* plan) const { return plan->reserved[0] == stamp_; }
    // the latest plan's device or host state is no longer what it planned: no exec may use it
    void invalidate() {
        if (++stamp_ == 0) ++stamp_;
    }

private:
    void drop_pairs() {
        pair_class.release();
        pair_status.release();
        large_ids.release();
        large_info.release();
        fresh_recs.release();
        redo_ids.release();
    }
    uint32_t stamp_ = 1;
};

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

}  // namespace pvhip

struct pvac_hip_ctx {
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    pvac_hip_params prm{};
    uint32_t layer_limit = PVAC_LAYER_LIMIT_DEFAULT;   // pvac_hip_ctx_set_layer_limit (a chain worker: its parent's)
    // pvac_hip_deep_route_count: lincomb terms on the deep-term route, lincomb fold sums run by k_ct_add_deep,
    // compact ciphers and recrypt sums above kAddLdsLayers layers
    uint64_t deep_route[4] = {};
    std::string err;
    pvhip::dev_buf<uint32_t> nb_table;  // libstdc++ bucket counts and their fastmod64 multipliers
    pvhip::dev_buf<uint64_t> nb_magic;
    pvhip::plan_scratch ps;
    pvhip::dev_buf<uint64_t> scan_scratch;
    void* pin = nullptr;   // pinned host words for the plan's and exec's read-backs (hipHostFree in ctx_destroy)
    pvhip::dev_buf<uint64_t> powg;   // pk.powg_B on the device, B x (lo, hi)
    uint32_t powg_n = 0;
    pvhip::sigma_tables H;
    uint64_t H_gen = 0;              // bumped whenever H is set (a worker's copy follows it)
    uint8_t H_digest[32] = {0};      // pk.H_digest
    bool have_digest = false;
    pvhip::dev_buf<unsigned long long> commit_counter;   // commit_ct: the cipher index its lanes draw from

    struct {   // ct_mul (rt_mul.cpp): the fresh kernel's arguments, the general path, counters
        pvhip::dev_buf<pvhip::mul_fresh_args> fresh_args;   // device copy of the fresh kernel's arguments
        pvhip::mul_fresh_args fresh_args_host{};
        bool fresh_args_uploaded = false;            // the device copy holds fresh_args_host
        pvhip::dev_buf<uint32_t> salt_pos;
        std::vector<pvhip::large_desc> set;          // the latest plan's general-path pairs, in pair order
        pvhip::sub_batch sub;                        // the sub-batch being launched (run_large)
        pvhip::dev_buf<pvhip::large_desc> desc_dev;
        pvhip::dev_buf<uint32_t> sel_dev;            // products: descriptor order per sub-batch (sub_batch::sel)
        pvhip::dev_buf<uint32_t> arena;              // in 32-bit words
        // static bucket-group tables of the last plan (one per distinct bucket count) + build scratch
        pvhip::dev_buf<uint32_t> grp, grp_tmp;
        pvhip::dev_buf<uint64_t> img_tmp;            // image -> records: 3 words per edge of the pairs converted
        pvhip::dev_buf<uint64_t> img_pairs;          // [2 n]: pair ids, then their offsets in img_tmp
        uint64_t last_pairs = 0;     // pairs of the last ct_mul_exec (pair_status is valid for these)
        uint64_t redo_total = 0;     // pairs re-run by redo_fresh_pairs since the context was created
        uint64_t path_total[4] = {}; // pair launches: fresh kernel, general path, its iblk order, direct mode
        uint64_t deep_total = 0;     // ... and of the general path's, the deep kernels (k_large_deep.hip)
    } mul;
    struct {   // the over-budget merge path of ct_add and compact (rt_add.cpp)
        std::vector<pvhip::merge_pair_info> set;     // the latest add or compact plan's items, in pair order
        pvhip::dev_buf<uint8_t> scratch;
        pvhip::dev_buf<unsigned long long> counters;
        pvhip::dev_buf<uint64_t> zero_n;             // zero words: the counts of compact's empty B
        pvhip::dev_buf<uint32_t> deep_slab;          // k_ct_add_deep: a keep / remap word per layer slot of the plan
        uint64_t deep_calls = 0;                     // ct_add / ct_sub calls run by k_ct_add_deep
    } merge;
    struct {   // LPN PRF key material (SecKey), enc_value and dec_value scratch (rt_keys.cpp)
        uint64_t k[4] = {0, 0, 0, 0};
        pvhip::dev_buf<uint64_t> lpn_s;
        uint32_t lpn_words = 0, lpn_t = 0, tau_num = 0, tau_den = 0;
        bool have_secret = false;
        bool aes_tables = false;
        pvhip::dev_buf<uint8_t> req;
        pvhip::dev_buf<uint64_t> core;
        pvhip::dev_buf<uint8_t> enc_arena;
        double noise_bits = 120.0, noise_t2 = 0.55, noise_slope = 16.0;   // Params noise fields (enc plan_noise)
        pvhip::dev_buf<uint8_t> dec_scratch;
        pvhip::dev_buf<uint64_t> dec_roff;
        uint32_t enc_plan_limit = PVAC_ENC_PLAN_LIMIT_DEFAULT;   // pvac_hip_ctx_set_enc_plan_limit
        uint64_t enc_budget = PVAC_ENC_BUDGET_DEFAULT;           // pre-merge edges of a sub-batch
        uint64_t enc_path[4] = {};   // items narrow / wide, sub-batches and calls (pvac_hip_enc_path_count)
    } prf;
    struct {   // ct_recrypt and its parts (rt_recrypt.cpp, k_recrypt.hip)
        pvhip::dev_buf<uint32_t> ubk_perm;           // pk.ubk as a gather: perm[inv[src]] = src (set_ubk)
        bool have_ubk = false;
        uint64_t compact_path[2] = {};               // ciphers compacted by k_compact_small / by the merge path
        pvhip::dev_buf<uint64_t> idx;                // per-iteration offset / count views and popcounts
        pvhip::dev_buf<uint32_t> ids;                // cipher ids of a view
        struct set {                                 // one of the two intermediate batches
            pvhip::dev_buf<pvac_layer> layers;
            pvhip::dev_buf<uint64_t> meta, w_lo, w_hi, sigma;
        } buf[2];
    } recrypt;
    struct {   // ct_lincomb (rt_lincomb.cpp, k_lincomb.hip)
        pvhip::dev_buf<uint64_t> terms;              // the latest plan's five per-term arrays, n_terms + 1 words each
        pvhip::dev_buf<uint32_t> tseg, remap, cls, tile_l, tile_e;
        pvhip::dev_buf<uint8_t> troute;
        pvhip::dev_buf<uint64_t> wg_ids, fold_ids;
        pvhip::dev_buf<uint64_t> route_ids;          // a plan with a deep term: two counts, then wg_ids split by route
        uint64_t n = 0, n_terms = 0, n_wg = 0, n_deep = 0, n_fold = 0;   // ... and its shape
        uint64_t status_n = 0;                       // segments of the last exec (cls holds their status)
        uint64_t path[4] = {};                       // segments one-pass / fold, terms wave / workgroup route
        struct set {                                 // the fold route's accumulator, ping-pong
            pvhip::dev_buf<pvac_layer> layers;
            pvhip::dev_buf<uint64_t> meta, w_lo, w_hi, sigma;
        } acc[2];
        pvhip::dev_buf<uint64_t> sw_lo, sw_hi;       // a scaled term's weights
        pvhip::dev_buf<uint64_t> words;              // zero offsets, the accumulators' counts, a plan's offsets
    } lincomb;
    struct {   // check_mul_gsum (rt_util.cpp)
        pvhip::dev_buf<unsigned int> buf;        // 4 layer maxima, then a u64 failure count
        pvhip::dev_buf<uint8_t> scratch;         // layer tables beyond LDS (global slabs)
        uint64_t path[2] = {};                   // calls with the tables in LDS / in global slabs
    } check;
    struct {   // sigma_bytehist / layer_gsum (rt_metrics.cpp, k_metrics.hip)
        pvhip::dev_buf<unsigned long long> sizes;   // layer_gsum's size pass, then the slab ticket
        pvhip::dev_buf<uint8_t> slabs;              // layer tables beyond LDS
        uint64_t path[5] = {};                      // bytehist calls wide / strided; gsum ciphers wave / workgroup / large
    } metrics;
    struct {   // the device .ct codec (rt_codec.cpp, k_ct_image.hip)
        pvhip::dev_buf<uint64_t> sz, toff;          // the latest image plan: size scratch, edge tile offsets
        pvhip::dev_buf<uint64_t> words;             // a parse's counts, offsets and tile offsets
        pvhip::dev_buf<unsigned long long> ctl;     // kCtImageCtlWords
        const uint64_t* plan_pos = nullptr;         // the latest image plan (null: none): its pos array,
        uint64_t plan_n = 0, plan_bytes = 0, plan_tiles = 0;   // ... shape and totals
        uint32_t plan_nbits = 0, plan_tile_edges = 0;
        uint64_t path[4] = {};                      // writes wide / 8-byte sigma path, parses wide / 8-byte
    } codec;
    struct {   // pvac_hip_batch_gather (rt_gather.cpp, k_gather.hip): storage of its own, so no other plan goes stale
        pvhip::dev_buf<uint64_t> words;             // the latest plan's eight per-output arrays (gather_plan_args)
        pvhip::dev_buf<uint32_t> src;               // ... and the source of every output cipher
        pvhip::dev_buf<uint64_t> table;             // the uploaded source descriptors, then their first outputs
        pvhip::dev_buf<unsigned long long> ctl;     // kGatherCtlWords
        std::vector<pvac_ct_batch> srcs;            // the latest plan (planned: there is one): its sources,
        std::vector<uint64_t> first;                // their first outputs in a concatenation,
        bool planned = false;
        uint64_t m = 0, total_layers = 0, total_edges = 0;   // its shape and totals,
        uint64_t tiles = 0, tiles_sigma = 0;        // its tiles without and with sigma rows of
        uint32_t sigma_words = 0;                   // the sources' common width (0: they cannot give sigma),
        const uint32_t* pick_src = nullptr;         // its pick lists
        const uint64_t* pick_idx = nullptr;
        const uint64_t* dst_index[4] = {};          // and dst's l_off, l_cnt, e_off, e_cnt
        uint64_t path[4] = {};                      // execs wide / 8-byte sigma path, tiles dealt, output ciphers
    } gather;
    struct {   // the CTR_DRBG behind pvac_hip_drbg_* (rt_drbg.cpp, drbg.hpp, k_drbg.hip)
        pvhip::ctr_drbg gen;            // its own mutex guards the state
        uint64_t epoch = 0;             // bumped by pvac_hip_drbg_seed (a chain worker's generator follows it)
        uint64_t worker_from = ~0ull;   // a chain worker: the parent's epoch its seed was drawn at (~0: not yet)
    } drbg;
    struct {
        bool on = false;
        std::map<std::string, pvhip::timer_rec> timers;
        std::vector<hipEvent_t> ev_pool;   // timer events returned by flush_timers, reused (no create per launch)
    } timing;
    struct {   // pvac_hip_ct_mul_chain, the caller's context: its workers (own stream / arena)
        std::vector<pvac_hip_ctx*> kids;   // [range j * streams + w] of the last call's layout
        std::vector<int64_t> layout;       // the last call's (streams, chunk, n_devices, ordinals...)
    } chain;
    struct {   // ... and what a worker context holds; the scalars keep their defaults in any other context
        pvhip::chain_set bufs[2];
        pvhip::chain_set stage;                    // staged chunk inputs (another device, or STAGE)
        pvhip::chain_set stage_op;                 // ... and the staged per-step operand (pvac_chain_opts::operands)
        pvhip::dev_stream_buf<uint64_t> nonces;
        pvhip::dev_stream_buf<uint64_t> salts;     // final-step salts (WITH_SIGMA)
        pvhip::dev_stream_buf<uint64_t> out;       // digests / counts of a chunk before the copy to X's device
        pvhip::dev_buf<unsigned long long> stats;  // [2 * PVAC_CHAIN_MAX_DEPTH + 1]: edges / products, image pair-steps
        uint64_t arena_cap_words = 0;   // general-path scratch cap in words (0 = half the free HBM): workers share the device
        uint32_t img_grid_y = 65535;    // pairs per image -> records launch (PVAC_CHAIN_IMG_BATCH2: 2)
        uint32_t spin_us = 50000;       // read_back's spin before a blocking wait (workers: 200)
        uint64_t H_from = 0;            // the parent's H_gen this context's H copy was taken from
        // the stream-ordered buffers go back on the context's stream; the caller synchronises
        void release(hipStream_t st) {
            for (pvhip::chain_set* b : {&bufs[0], &bufs[1], &stage, &stage_op}) b->release(st);
            nonces.release(st);
            salts.release(st);
            out.release(st);
        }
    } worker;
};

namespace pvhip {

inline int fail(pvac_hip_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

inline int hip_fail(pvac_hip_ctx* c, hipError_t e, const char* where) {
    if (e == hipSuccess) return PVAC_OK;
    std::string m = std::string(where) + ": " + hipGetErrorString(e);
    return fail(c, e == hipErrorOutOfMemory ? PVAC_ENOMEM : PVAC_EDEVICE, m);
}

// The one exception boundary. Every extern "C" entry that can allocate on the host (a std::vector, a
// map node, an error message) is a function-try-block whose handler is
//     } catch (...) { return caught(c, "<entry>"); }
// and a chain worker's thread body runs under guarded(). Called inside a handler, caught() maps the
// exception in flight: a std::exception becomes PVAC_ENOMEM with "<entry>: <what()>"; c may be null.
// Nothing leaves it.
inline int caught(pvac_hip_ctx* c, const char* entry) noexcept {
    try {
        throw;
    } catch (const std::exception& ex) {
        try {
            return fail(c, PVAC_ENOMEM, std::string(entry) + ": " + ex.what());
        } catch (...) {
        }
    } catch (...) {
    }
    if (c) c->err.clear();   // no memory for the message either
    return PVAC_ENOMEM;
}

template <class F>
int guarded(pvac_hip_ctx* c, const char* entry, F&& body) noexcept {
    try {
        return body();
    } catch (...) {
        return caught(c, entry);
    }
}

struct scoped_timer {
    pvac_hip_ctx* c;
    timer_rec* rec = nullptr;
    hipEvent_t a{}, b{};
    scoped_timer(pvac_hip_ctx* ctx, const char* name) : c(ctx) {
        if (!c->timing.on) return;
        rec = &c->timing.timers[name];
        a = take();
        b = take();
        hipEventRecord(a, c->stream);
    }
    hipEvent_t take() {
        hipEvent_t e{};
        if (!c->timing.ev_pool.empty()) {
            e = c->timing.ev_pool.back();
            c->timing.ev_pool.pop_back();
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

// The short host waits of a plan (its totals) and of exec (the redo count): a blocking
// hipStreamSynchronize wakes tens of microseconds after the copy lands, so spin on hipStreamQuery
// (up to spin_us, then block) and read into pinned words (a pageable destination stages the copy).
// A caller's context spins up to 50 ms (one thread, the headline step); the chain's worker contexts
// (several threads per device) spin 200 us and then block, so they do not hold cores and the HIP
// runtime's locks while their kernels run.
inline hipError_t read_back(pvac_hip_ctx* c, void* dst, const void* src, size_t bytes) {
    if (c->pin && bytes <= 256) {
        hipError_t e = hipMemcpyAsync(c->pin, src, bytes, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) return e;
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            e = hipStreamQuery(c->stream);
            if (e != hipErrorNotReady) break;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(c->worker.spin_us)) {
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

// n words to the device on the context's stream, waited for: the host words may change afterwards
inline hipError_t upload_words(pvac_hip_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!bytes) return hipSuccess;
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e;
}

// the exclusive scans' scratch for n counts; it is no plan's state, so a pending plan stays valid
inline int ensure_scan(pvac_hip_ctx* c, size_t n) {
    const size_t sw = scan_scratch_words(n);
    return hip_fail(c, c->scan_scratch.grow(sw, sw), "alloc scan scratch");
}

inline bool batch_ok(const pvac_ct_batch* X) {
    return X && (X->n == 0 || (X->l_off && X->l_cnt && X->e_off && X->e_cnt));
}

inline bool sigma_ok(const pvac_hip_ctx* c, const pvac_ct_batch* X) {
    return X->sigma && X->sigma_words >= (c->prm.m_bits + 63) / 64;
}

// The pass every plan starts with: a new stamp over scratch for n items, the stats zeroed, the plan
// kernel (`launch`, which returns its hipError_t), with `scan` the exclusive scans of C's offsets,
// and the stats read back into st.
template <class Launch>
int plan_pass(pvac_hip_ctx* c, uint64_t n, pvac_ct_batch* C, bool scan, const char* where, Launch&& launch, plan_stats& st) {
    plan_scratch& ps = c->ps;
    const size_t cap0 = ps.capacity();
    int rc = hip_fail(c, ps.begin(n), "alloc pair scratch");
    // regrown (or given back) arrays no longer hold the last ct_mul_exec's pair_status: ct_mul_status
    // refuses until the next exec instead of copying out words no kernel wrote
    if (ps.capacity() != cap0) c->mul.last_pairs = 0;
    if (!rc) rc = ensure_scan(c, n);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync(ps.stats.get(), 0, sizeof(plan_stats), c->stream);
    if (e == hipSuccess) e = launch();
    if (e == hipSuccess && scan)
        e = launch_exclusive_scan2_u64(C->l_off, C->e_off, n, c->scan_scratch.get(), &ps.totals[0], &ps.totals[1], c->stream);
    st = plan_stats{};
    if (e == hipSuccess) e = read_back(c, &st, ps.stats.get(), sizeof st);
    return hip_fail(c, e, where);
}

// a plan's totals, classes and launch maxima from the stats of its pass over n items (a plan kernel
// leaves the maxima it does not compute at 0)
inline void plan_fill(pvac_hip_plan* plan, uint64_t n, const plan_stats& st) {
    plan->total_layer_slots = st.total_layers;
    plan->total_edge_slots = st.total_edges;
    plan->n_small = n - st.n_large;   // a plan kernel classifies every item as small or large
    plan->n_large = st.n_large;
    plan->max_keys = st.max_keys;
    plan->max_prod = st.max_prod;
    plan->max_na = st.max_na;
    plan->max_nb = st.max_nb;
    plan->max_buckets = st.max_buckets;
    plan->max_layers = st.max_layers;
}

// ---------------------------------------------------------------- across the units
// A chain step's dense images (pvac_hip_ct_mul_chain; mul_large_args::A_img / C_img): per-pair flags
// of A (read; cleared where A is turned back into records) and of C (written), and the counter of
// pair-steps written as images. All null outside the chain.
struct step_images {
    uint32_t* in = nullptr;
    uint32_t* out = nullptr;
    unsigned long long* count = nullptr;
};

// rt_mul.cpp: pvac_hip_ct_mul_exec, with a chain step's images (all null for a caller's batch)
int ct_mul_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* A, const pvac_ct_batch* B,
                const uint64_t* nonces, const uint64_t* salts, pvac_ct_batch* C, uint32_t flags, step_images img);

// rt_drbg.cpp: n words of the context's generator into out on the context's stream (pvac_hip_drbg_fill)
int drbg_fill(pvac_hip_ctx* c, uint64_t* out, size_t n_words, const char* where);

// rt_add.cpp: pvac_hip_ct_add_exec with the most layers a pair may have. The ABI entry and the sums of
// ct_recrypt and ct_lincomb all pass deep_layer_bound(the context's layer limit) (deep_ops.hpp)
constexpr uint32_t kAddLdsLayers = 30000;   // |A.L| + |B.L| k_ct_add's LDS keep table holds (120 KB)
static_assert(kAddLdsLayers == kLinMaxLayers, "one bound for every LDS keep table");
int ct_add_exec(pvac_hip_ctx* c, const pvac_hip_plan* plan, const pvac_ct_batch* A, const pvac_ct_batch* B, int negate_b,
                pvac_ct_batch* C, uint32_t lmax);

// rt_add.cpp, the merge set: the over-budget items ids[0, n) of the plan just made, 8 words each from
// `gather` (into the device array it is given), turned into c->merge.set in pair order by `decode`
// (false = beyond the caller's limits: limit_msg, PVAC_ENOSYS); then one launch_add_merge per item
int merge_gather(pvac_hip_ctx* c, uint64_t n, const std::function<hipError_t(uint64_t*)>& gather,
                 const std::function<bool(const uint64_t*, merge_pair_info&)>& decode, const char* where,
                 const char* limit_msg);
int merge_execute(pvac_hip_ctx* c, const pvac_ct_batch& A, const pvac_ct_batch& B, pvac_ct_batch& C, int negate_b,
                  const char* where);

}  // namespace pvhip
