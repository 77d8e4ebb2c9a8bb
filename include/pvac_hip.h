/* pvac_hip.h — C ABI of the MI355X (gfx950) batched ciphertext-arithmetic engine.
 *
 * Drop-in boundary for the pvac-hfhe 0.1.0 hot path (reference: include/pvac/...). The
 * reference exposes a header-only, by-value C++ API and no FFI; every entry point below
 * names the reference function it replaces. The C++ adapter include/pvac_hip.hpp is
 * templated on the reference's own pvac::Cipher / PubKey types (it does not restate them) and
 * routes batched calls through these entry points; INTEGRATION.md §2 is the patch a
 * maintainer adds to the reference's ops/arithmetic.hpp to dispatch ct_mul & co. through it.
 *
 * Conventions
 *  - All functions are noexcept, never throw, and return int status: 0 = ok, <0 = error
 *    (PVAC_E*); pvac_hip_last_error(ctx) gives a message.
 *  - Pointers inside batches/arrays are DEVICE pointers (hipMalloc / torch CUDA tensors)
 *    unless a parameter says "host". Work is enqueued on the ctx stream; functions that
 *    must return sizes to the host synchronise that stream (documented per function).
 *  - One thread per ctx. Contexts are independent (one per device / per host thread).
 *  - Fp values are p = 2^127-1 field elements as two u64 limbs (lo, hi) in SoA arrays.
 *  - Randomness is an explicit input: the reference draws nonces/salts from getrandom(2)
 *    inside ct_mul (core/random.hpp:40-110); here the caller passes those words, which
 *    makes outputs reproducible and testable. The C++ adapter fills them from getrandom.
 */
#ifndef PVAC_HIP_H
#define PVAC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVAC_HIP_ABI_VERSION 3

/* status codes */
#define PVAC_OK 0
#define PVAC_EINVAL (-22)
#define PVAC_ENOMEM (-12)
#define PVAC_ENOSYS (-38)
#define PVAC_EDEVICE (-5)
#define PVAC_ERANGE (-34)

/* fp binop codes (core/field.hpp:50-71,209-213; ops/arithmetic.hpp:33-37 for SCALE) */
#define PVAC_FP_ADD 0
#define PVAC_FP_SUB 1
#define PVAC_FP_MUL 2
#define PVAC_FP_NEG 3   /* b ignored */
#define PVAC_FP_SCALE 4 /* b is ONE element, broadcast: c[i] = a[i] * b[0] */
#define PVAC_FP_INV 5   /* fp_inv (field.hpp:229-273) = a^(p-2), inv(0) = 0; b ignored */

/* ct_mul flags */
#define PVAC_MUL_WITH_SIGMA 0x1u      /* also generate per-edge sigma (crypto/matrix.hpp:267-303) */
#define PVAC_MUL_ORDER_CANONICAL 0x2u /* emit (layer, idx, P<M) sorted instead of the reference hash order */

typedef struct pvac_hip_ctx pvac_hip_ctx;

/* Mirrors the subset of pvac::Params + PubKey that the hot path reads
 * (core/types.hpp:36-70, 121-129). */
typedef struct pvac_hip_params {
    uint32_t B;          /* 337 */
    uint32_t m_bits;     /* 8192: sigma bits */
    uint32_t n_bits;     /* 16384: H columns */
    uint32_t h_col_wt;   /* 192 */
    uint32_t x_col_wt;   /* 128 */
    uint32_t err_wt;     /* 128 */
    uint64_t edge_budget;/* 1200000 (guard_budget, ops/encrypt.hpp:106-111) */
    uint64_t canon_tag;  /* pk.canon_tag */
} pvac_hip_params;

/* pvac::Layer (core/types.hpp:96-101) as a 40-byte record. rule: 0 = BASE, 1 = PROD. */
typedef struct pvac_layer {
    uint32_t rule, pa, pb, pad;
    uint64_t ztag, nonce_lo, nonce_hi;
} pvac_layer;

/* A batch of n ciphers (pvac::Cipher, core/types.hpp:116-119), SoA with per-cipher
 * (offset, count) ranges so both dense CSR and capacity-padded outputs are expressible.
 * Edge meta packs pvac::Edge{layer_id, idx, ch} exactly like the .ct edge header:
 *   meta = layer_id | (u64)idx << 32 | (u64)ch << 48.
 * sigma (nullable) holds sigma_words u64 per edge slot (edge slot e -> sigma[e*sigma_words]). */
typedef struct pvac_ct_batch {
    uint64_t n;
    uint64_t* l_off;   /* [n] first layer slot of cipher i */
    uint64_t* l_cnt;   /* [n] layers of cipher i */
    pvac_layer* layers;
    uint64_t* e_off;   /* [n] first edge slot of cipher i */
    uint64_t* e_cnt;   /* [n] edges of cipher i */
    uint64_t* meta;
    uint64_t* w_lo;
    uint64_t* w_hi;
    uint64_t* sigma;
    uint32_t sigma_words;
    uint32_t pad;
} pvac_ct_batch;

/* Output sizing of a batched ct_mul / ct_add (filled by the *_plan calls). */
typedef struct pvac_hip_plan {
    uint64_t total_layer_slots;   /* sum of per-pair layer capacities */
    uint64_t total_edge_slots;    /* sum of per-pair edge capacities */
    uint64_t n_pairs;
    uint64_t n_small;             /* pairs served by the LDS-resident fresh-shape kernel */
    uint64_t n_large;             /* pairs served by the layer-dense path */
    uint64_t n_invalid;           /* reserved, always 0: rejections are per pair, see pvac_hip_ct_mul_status */
    uint32_t max_keys, max_prod, max_na, max_nb, max_buckets, max_layers;  /* launch sizing */
    uint32_t kind;                /* 1 = mul, 2 = add, 3 = sub, 4 = recrypt, 5 = compact, 6 = lincomb */
    uint32_t reserved[5];
} pvac_hip_plan;

/* ---------------------------------------------------------------- context */
int pvac_hip_abi_version(void);
/* Create a context on `device`. Replaces the implicit PubKey plumbing of the reference. */
int pvac_hip_ctx_create(int device, const pvac_hip_params* prm, pvac_hip_ctx** out);
int pvac_hip_ctx_destroy(pvac_hip_ctx* ctx);
/* Run on the caller's stream (e.g. torch.cuda.current_stream().cuda_stream); NULL = the legacy
 * null stream. A fresh context starts on a private non-blocking stream of its own. */
int pvac_hip_ctx_set_stream(pvac_hip_ctx* ctx, void* hip_stream);
void* pvac_hip_ctx_stream(pvac_hip_ctx* ctx);
int pvac_hip_ctx_synchronize(pvac_hip_ctx* ctx);
/* The noise fields of the reference's Params (core/types.hpp:48-50: noise_entropy_bits 120,
 * tuple2_fraction 0.55, depth_slope_bits 16 by default), used by enc_value / enc_value_depth's
 * plan_noise (ops/encrypt.hpp:16-27). A plan above 256 pre-merge edges per half is PVAC_ENOSYS. */
int pvac_hip_ctx_set_noise(pvac_hip_ctx* ctx, double noise_entropy_bits, double tuple2_fraction, double depth_slope_bits);
const char* pvac_hip_last_error(pvac_hip_ctx* ctx);
/* Upload the public parity matrix H (pk.H, crypto/matrix.hpp:191-251) from a HOST dense
 * array of n_bits columns x ceil(m_bits/64) words; stored on device as per-column sparse
 * row lists. Required only for PVAC_MUL_WITH_SIGMA / pvac_hip_sigma_batch. Synchronous. */
int pvac_hip_ctx_set_H(pvac_hip_ctx* ctx, const uint64_t* H_dense_host, uint32_t n_cols, uint32_t words_per_col);
/* Regenerate H on the device from params.canon_tag (gen_H, crypto/matrix.hpp:191-251) and
 * return its H_digest (host, 32 bytes). */
int pvac_hip_ctx_gen_H(pvac_hip_ctx* ctx, uint8_t digest_out[32]);

/* Measured integer-ALU ceilings of this device for the roofline report (k_ubench.hip), per second:
 * kind 0 = wave64 integer VALU instructions (v_mad_u64_u32 / v_add_co_u32 / v_alignbit_b32 mix),
 * 1 = lazy fp_mul_fold1 products, 2 = full fp_mul products, 3 = column-accumulated products
 * (col26_mac, the general path's dense loop), 4 = wave64 single-pass 32-bit VALU instructions
 * (v_add_u32 / v_xor_b32 / v_alignbit_b32: the issue ceiling of a mostly 32-bit VALU stream),
 * 5 = general-path dense-mode products on the matrix cores (v_mfma_i32_32x32x32_i8 rate x 64).
 * Synchronous. */
int pvac_hip_alu_ceiling(pvac_hip_ctx* ctx, int kind, double* per_s);
/* Per-opcode VALU issue probe (k_ubench.hip): one opcode alone on 16 independent accumulators per
 * lane, waves_per_simd (1..8) waves on every SIMD. Returns wave64 instructions per second chip-wide
 * and the shader clock the SIMDs ran at during the same launch (s_memtime ticks per s_memrealtime
 * tick x 100 MHz, median over workgroups), so cycles per instruction = SIMDs x clock / per_s.
 * op: 0 v_add_u32, 1 v_xor_b32, 2 v_alignbit_b32, 3 v_lshlrev_b32, 4 v_min_u32, 5 v_add3_u32,
 * 6 v_pk_add_u16, 7 v_fma_f32, 8 v_mul_lo_u32, 9 v_mul_hi_u32, 10 v_cndmask_b32, 11 v_bfe_u32,
 * 12 v_add_co_u32, 13 v_and_or_b32, 14 v_pk_min_u16, 15 v_bitop3_b32, 16 v_mad_u64_u32,
 * 17 v_cndmask_b32_e64 (SGPR-pair mask), 18 v_lshl_add_u32, 19 v_mov_b32 DPP row_shr, 20 v_perm_b32,
 * 21 v_mul_u32_u24, 22 v_sub_u32, 23 v_max3_u32, 24 v_cmp (VCC) + VOP2 v_cndmask_b32 pairs, 25 v_cndmask_b32_e64
 * reading VCC, 26 VOP2 v_addc_co_u32 (VCC carry), 27 v_addc_co_u32_e64 (SGPR carry), 28 v_cmp_e64 + v_cndmask_b32_e64
 * (SGPR mask) pairs, 29 v_min_u32_e64, 30 v_add_u32_e64, 31 v_and_b32, 32 v_or_b32, 33 v_lshrrev_b32,
 * 34 v_mov_b32, 35 v_max_u32, 36 v_add_u32_sdwa (byte source), 37 / 38 v_lshlrev_b32_sdwa (byte shifted / byte
 * shift count), 39 v_xor_b32_e64, 40 v_mad_u32_u24.
 * Measurement only (never used by an op). Synchronous. */
int pvac_hip_issue_probe(pvac_hip_ctx* ctx, int op, int waves_per_simd, double* per_s, double* clock_hz);
/* Per-kernel device timing (HIP events on the ctx stream) for the roofline report. */
int pvac_hip_timing_enable(pvac_hip_ctx* ctx, int on);
/* kernel_name: "fp_binop", "ct_mul_small", "ct_mul_large", "ct_add", "sigma", ... (the deep kernels:
 * "large_lists_deep", "large_layers_deep", both inside "ct_mul_large", and "ct_add_deep"); returns
 * accumulated milliseconds and launch count since the last reset (synchronises). */
int pvac_hip_timing_get(pvac_hip_ctx* ctx, const char* kernel_name, double* ms, uint64_t* launches);
int pvac_hip_timing_reset(pvac_hip_ctx* ctx);

/* ---------------------------------------------------------------- element-wise Fp
 * Replaces fp_add / fp_sub / fp_mul / fp_neg (core/field.hpp:50-71, 209-213) applied over
 * arrays; results are bit-identical to the reference including its quirks for non-canonical
 * inputs (fp_add truncates the high-word carry, field.hpp:53-55). In-place (c == a) allowed. */
int pvac_hip_fp_binop(pvac_hip_ctx* ctx, int op, const uint64_t* a_lo, const uint64_t* a_hi, const uint64_t* b_lo,
                      const uint64_t* b_hi, uint64_t* c_lo, uint64_t* c_hi, size_t n);

/* ---------------------------------------------------------------- batched ciphertext ops
 * ct_mul (ops/arithmetic.hpp:47-106) over n independent pairs C[i] = A[i] * B[i].
 * Two-phase sizing:
 *   1. pvac_hip_ct_mul_plan: writes C->l_off / C->e_off (device) with per-pair capacities
 *      (layers |A.L|+|B.L|+|A.L||B.L|, edges 2*min(|A.E||B.E|, |A.L||B.L|B)), zeroes C->l_cnt /
 *      C->e_cnt when given, and fills *plan (synchronises the stream once to read totals back).
 *   2. caller allocates C->layers (total_layer_slots), C->meta/w_lo/w_hi (total_edge_slots),
 *      optional C->sigma, then pvac_hip_ct_mul_exec writes C->l_cnt/e_cnt and the records.
 * Randomness (replaces the getrandom draws of arithmetic.hpp:59-70,90-94):
 *   nonces: 2 words per OUTPUT layer slot (device, parallel to C->layers): for the product
 *           layer of (la, lb) at slot l_off+|A.L|+|B.L|+la*|B.L|+lb, words [2s]=lo, [2s+1]=hi.
 *   salts : 1 word per OUTPUT edge slot (device, parallel to C->meta), in emit order; used only
 *           with PVAC_MUL_WITH_SIGMA (nullable otherwise).
 * Output edge order is the reference's std::unordered_map iteration order (bit-exact), unless
 * PVAC_MUL_ORDER_CANONICAL. guard_budget/compact_layers semantics are applied per pair.
 * exec synchronises the stream once at its end: a fresh-shape pair with a key sum of 0 mod p
 * (cancelling products, zero weights) is re-run on the general path before it returns. */
int pvac_hip_ct_mul_plan(pvac_hip_ctx* ctx, const pvac_ct_batch* A, const pvac_ct_batch* B, pvac_ct_batch* C,
                         pvac_hip_plan* plan);
int pvac_hip_ct_mul_exec(pvac_hip_ctx* ctx, const pvac_hip_plan* plan, const pvac_ct_batch* A, const pvac_ct_batch* B,
                         const uint64_t* nonces, const uint64_t* salts, pvac_ct_batch* C, uint32_t flags);
/* plan + exec in one call, into output arrays the caller sized once (for a stream of batches of
 * one shape, no host round trip between the two): C->l_off / e_off / l_cnt / e_cnt hold A->n,
 * C->layers layer_cap slots, C->meta / w_lo / w_hi (and C->sigma) edge_cap slots. When this plan
 * needs more, nothing is launched after it and the call returns PVAC_ENOMEM with *plan (nullable)
 * holding the sizes to allocate (the plan has rewritten C's offset and count arrays by then; C's
 * rows are untouched). nonces / salts as for pvac_hip_ct_mul_exec (the nonce slots are
 * C's planned layer slots, so they are valid only while the plan's offsets are: batches of one
 * shape plan the same offsets). */
int pvac_hip_ct_mul(pvac_hip_ctx* ctx, const pvac_ct_batch* A, const pvac_ct_batch* B, pvac_ct_batch* C,
                    uint64_t layer_cap, uint64_t edge_cap, const uint64_t* nonces, const uint64_t* salts,
                    uint32_t flags, pvac_hip_plan* plan);
/* Pairs that ct_mul_exec re-ran on the general path (see above) since the context was created. */
int pvac_hip_ct_mul_redo_count(pvac_hip_ctx* ctx, uint64_t* out);
/* Pair launches by path since the context was created (diagnostics and tests): out[0] the
 * LDS-resident fresh-shape kernel, out[1] the general path (redo launches included), out[2] of
 * those the per-A-edge emit order, out[3] the direct mode (positions from key presence). */
int pvac_hip_ct_mul_path_count(pvac_hip_ctx* ctx, uint64_t* out);
/* The layer limit of a context. A ct_mul pair is accepted while its layers before compaction,
 * |A.L| + |B.L| + |A.L||B.L|, are at most the limit (PVAC_ENOSYS above it; the bounds |A.L||B.L|B < 2^31
 * and |A.E||B.E| < 2^32 hold at any limit), and ct_add / ct_sub while the largest |A.L| + |B.L| of the
 * batch is at most max(30000, limit). Up to PVAC_LAYER_LIMIT_DEFAULT layers (ct_add: 30000) the per-layer
 * tables of a pair live in LDS; a pair above runs the deep kernels (k_large_deep.hip), which keep them in
 * the pair's global scratch and change no result. The default is kept on purpose: the general path's
 * scratch is about 16 words per key slot (|A.L||B.L|B slots), at most ~350 MB at the default limit and
 * over 100 GB near 2^31 slots, so a caller raises the limit knowing what its ciphers cost.
 * set: PVAC_EINVAL outside [PVAC_LAYER_LIMIT_DEFAULT, PVAC_LAYER_LIMIT_MAX]. The workers of
 * pvac_hip_ct_mul_chain take the calling context's limit at each call. The 30000-layer refusals of
 * ct_lincomb, compact and ct_recrypt move with the limit as ct_add's does: a lincomb term (and a fold-route
 * segment in all), a cipher compact hands to its merge path and a ct_recrypt sum (a cipher plus a pool
 * member) may have max(30000, limit) layers. Above 30000 a lincomb term is closed by the deep-term
 * route, whose keep and remap words are in global scratch (4 bytes per input layer of the call), and the
 * sums of the fold route and of ct_recrypt run k_ct_add_deep. An over-budget ct_add pair (guard_budget) and a cipher of
 * compact beyond its batched kernel take the merge kernel at any depth: it never builds the 2|L|B key
 * space, its scratch is 56 bytes per input edge (the 32-bit sort keys and values, in and out, and
 * five 8-byte columns) plus 4 bytes per layer and the radix sort's own temporary storage. */
#define PVAC_LAYER_LIMIT_DEFAULT 16384u
#define PVAC_LAYER_LIMIT_MAX (1u << 24)
int pvac_hip_ctx_set_layer_limit(pvac_hip_ctx* ctx, uint32_t max_layers); /* DEFAULT..MAX, else PVAC_EINVAL */
int pvac_hip_ctx_layer_limit(pvac_hip_ctx* ctx, uint32_t* out);
/* Since the context was created: out[0] = ct_mul pairs run by the deep kernels (a chain's workers
 * included), out[1] = ct_add / ct_sub calls run by the deep kernel. */
int pvac_hip_deep_path_count(pvac_hip_ctx* ctx, uint64_t out[2]);
/* Since the context was created: out[0] = ct_lincomb terms planned on the deep-term route (counted by
 * exec, like pvac_hip_ct_lincomb_path_count), out[1] = sums of ct_lincomb's fold route handed to
 * k_ct_add_deep (they are counted in pvac_hip_deep_path_count's out[1] as well), out[2] = ciphers of more
 * than 30000 layers compacted (compact_exec and ct_recrypt_exec), out[3] = ct_recrypt's sums of more than
 * 30000 layers (|cipher.L| + |pool member.L|, per cipher and iteration). All zero at the default limit. */
int pvac_hip_deep_route_count(pvac_hip_ctx* ctx, uint64_t out[4]);
/* Per-pair outcome of the last ct_mul_exec, copied (stream-ordered) to the DEVICE array out[n]:
 * 0 = reference hash order, 1 = canonical (layer, idx, P<M) order (guard_budget or
 * PVAC_MUL_ORDER_CANONICAL), 2 = rejected. Rejection is stricter than the reference: an edge with
 * layer_id >= |X.L| (undefined behaviour there: C.L[lid] out of range), idx >= B or ch > 1
 * (defined there, out of the Cipher contract: dec_value indexes powg_B[idx]) makes the pair's
 * output empty (l_cnt = e_cnt = 0) instead. The statuses live in the per-pair plan scratch: a later plan
 * (ct_mul, ct_add, compact, ct_lincomb, ct_recrypt) of more pairs than the scratch held regrows it and
 * discards them, and the call then fails with PVAC_EINVAL, as it does for n above the last exec's
 * pairs, until the next ct_mul_exec. */
int pvac_hip_ct_mul_status(pvac_hip_ctx* ctx, uint32_t* out, size_t n);
/* The reference's ct_mul invariant check_mul_gsum_all (utils/metrics.hpp:88-113) on every pair of
 * a batch: gsum(C, product layer of (la, lb)) == gsum(A, la) * gsum(B, lb) with
 * gsum(X, l) = sum of +/- w * powg_B[idx] over X's edges in layer l (metrics.hpp:70-86). C is a
 * ct_mul_exec output of (A, B) with `nonces`: a product layer is identified by the nonce it
 * carries (compact_layers renumbers C's layers); a dropped product layer must have a zero product.
 * A C layer with edges must carry the nonce of exactly one product slot and have rule 1 (PROD);
 * edges whose layer_id is outside their cipher's layers are ignored, as by the reference's loops.
 * Needs pvac_hip_ctx_set_powg. status (nullable, DEVICE, n u32): 0 holds, 1 violated, 2 an edge
 * of A, B or C with idx >= B, 3 a cipher of 2^21 edges or more (not checked: the per-layer sums are
 * taken over 43/42/42-bit limbs in u64: n terms of at most 2^43 - 1 stay below 2^64 up to n = 2^21
 * and can pass it from 2^21 + 1, and the check refuses from 2^21 on; 3 wins over 2, 2 over 1).
 * *n_bad (host) = pairs with status != 0. Synchronous.
 * Tables: per pair the check keeps seven arrays, each rounded up to 16 bytes: 16 B bytes of powg
 * words; 48 |A.L|, 48 |B.L| and 48 |C.L| bytes of layer sums; 4 |C.L| bytes of edge counts; 16 and
 * 4 bytes per product slot (|A.L||B.L| slots). With the batch's maxima of |A.L|, |B.L|, |C.L| and
 * |A.L||B.L| (each taken on its own) their total decides the mode of the whole call: up to 163,824
 * bytes (a workgroup's 160 KiB of LDS less 16 bytes of the kernel's own state) the tables live in
 * LDS, one workgroup per pair over min(n, 8 x CU count) workgroups; above, in per-workgroup slabs
 * of global scratch over min(n, 2 x CU count) workgroups. Both modes compute the same statuses. */
int pvac_hip_check_mul_gsum(pvac_hip_ctx* ctx, const pvac_ct_batch* A, const pvac_ct_batch* B, const pvac_ct_batch* C,
                            const uint64_t* nonces, uint32_t* status, uint64_t* n_bad);
/* pvac_hip_check_mul_gsum calls on this context since it was created (diagnostics and tests) that
 * ran to completion with n > 0: out[0] with the tables in LDS, out[1] in global slabs. The checks
 * of pvac_hip_ct_mul_chain run on its workers' contexts and are not counted here. */
int pvac_hip_check_mul_gsum_path_count(pvac_hip_ctx* ctx, uint64_t out[2]);

/* ---------------------------------------------------------------- depth chains
 * c_0 = X[i], c_k = ct_mul(c_{k-1}, X[i]) for k = 1..depth, for every input i of X: the reference's
 * chain workload (tests/test_main.cpp:289-295, c = ct_mul(pk, c, x) in a loop) over a batch of
 * independent inputs. The library cuts X into chunks of `chunk` inputs and runs them on `streams`
 * worker threads, each with its own HIP stream, scratch arena and output buffers (child contexts
 * kept by ctx between calls), chunks handed out in input order. One chunk's host planning (the
 * plan's shape read-back) and its short dependent launches overlap other chunks' kernels, so a
 * single caller thread gets the concurrency. Synchronous: returns when every chunk is done.
 * Memory: each worker holds two output batches sized for its chunk's largest step (24 B per edge
 * slot; a depth-8 chain of enc_value inputs ends near 345 K edges, ~8.3 MB) plus a scratch arena
 * of at most half the free HBM over streams (an output array that does not fit takes the worker's
 * arena back first); streams x chunk beyond the device's HBM fails with PVAC_ENOMEM ("alloc edges"). A call whose (streams, n_devices, chunk) differ from the previous
 * call's first releases the workers' buffers and arenas.
 * Each step is exactly pvac_hip_ct_mul_plan + pvac_hip_ct_mul_exec (weights only, reference hash
 * order unless flags has PVAC_MUL_ORDER_CANONICAL). With PVAC_MUL_WITH_SIGMA the FINAL step also
 * gets its sigmas (sigma_from_H per output edge, arithmetic.hpp:90-94; the context needs H): the
 * reference draws one salt per emitted edge at every step, but only c_depth's sigmas survive (an
 * output sigma depends on its layer seed, idx, ch and salt alone), so intermediate steps stay
 * weights-only and a caller replaying a reference stream skips their salts (after_step gives the
 * counts). The final chunk buffer then holds 1 KiB of sigma per edge: size `chunk` for it.
 * Nonces: fill_nonces(user, step, first_input, n_words, dev_words, stream) when given (called on
 * the worker thread; fill n_words device words on `stream`, the 2-words-per-output-layer-slot
 * array of pvac_hip_ct_mul_exec), else splitmix64 words: pvac_hip_fill_random with seed
 * nonce_seed + 97 * first_input + step (step counted from 0). That default is a test stream.
 * PVAC_CHAIN_DRBG: with fill_nonces and nonces_at null, a step's nonce words come from the worker's
 * CTR_DRBG (pvac_hip_drbg_fill on the worker's context) instead; with PVAC_MUL_WITH_SIGMA and
 * salts_at null so do the final step's salts. Hooks, when given, still win; without the flag nothing
 * changes. Each worker context owns a generator, seeded with 48 bytes drawn from ctx's generator when
 * the worker is created (and again after ctx's generator is seeded anew by pvac_hip_drbg_seed).
 * Chunks are handed to workers dynamically, so a run with the flag is not reproducible at
 * streams > 1 even under an explicit seed; at streams = 1 it is.
 * Outputs are streamed: on_chunk(user, first_input, C, stream) receives each chunk's final
 * c_depth (device batch, capacity-padded CSR) valid until it returns; digest_out (DEVICE, nullable)
 * receives pvac_hip_batch_digest of c_depth for inputs [0, digest_n) (FNV-1a: serial over a cipher's
 * edges, ~0.2 s for a chunk of depth-8 chains), count_out (DEVICE, nullable) |E| of c_depth for
 * inputs [0, count_n).
 * PVAC_CHAIN_CHECK_GSUM runs the reference's gsum invariant (pvac_hip_check_mul_gsum) on every pair
 * of every step (needs pvac_hip_ctx_set_powg). A callback's nonzero return stops the chain with
 * PVAC_EINVAL.
 * Step hooks (all optional, called on the worker thread with the worker's stream; A = c_{step},
 * X = the chunk's inputs, C = c_{step+1}, all device batches valid during the call):
 *   (with per-step operands, below, X is the step's operand)
 *   nonces_at  before step `step`'s exec: fill dev_words[0, n_words) (2 words per layer slot of C,
 *              product layer (la, lb) of pair i at C.l_off[i] + |A_i.L| + |X_i.L| + la |X_i.L| + lb,
 *              lo then hi). Replaces fill_nonces.
 *   after_step after step `step`'s exec (C's weights, counts and layers are final; dev_words null).
 *   salts_at   WITH_SIGMA, final step, after its weights: fill dev_words[0, n_words) (n_words = C's
 *              edge slots): dev_words[C.e_off[i] + k] is the salt of pair i's k-th emitted edge in
 *              the reference's emit order (hash order; a pair in the canonical order still takes its
 *              salts in hash order, as pvac_hip_ct_mul_exec does).
 * Intermediate layout: without an after_step hook or the gsum check, a step from the third on whose
 * C is dense (every cell of every product layer present, under 2^21 edges) hands C to the next step
 * as a dense image instead of hash-order records: C's counts, offsets and layer records are final,
 * but edge slot s of pair i holds the weight of cell s mod 2B of its s / 2B-th product layer, and
 * 32-bit word s of the pair's meta region holds that edge's hash-order position | cell << 21
 * (stats.image_steps counts such pair-steps). The
 * next step reads it in place (no per-layer edge gathers); a pair that leaves the direct mode gets
 * its records back first. So nonces_at / salts_at may see A in that layout: read its counts and
 * layers only. c_depth (on_chunk, digests) is always records.
 * Devices: with n_devices > 0 the inputs are split into n_devices contiguous ranges of whole chunks
 * (by global input index; a range never splits a chunk, so every chunk, its nonce seeds and its
 * results are those of a one-device run) and each range runs on `streams` worker threads on
 * devices[j] (an ordinal may repeat). A worker whose device is not X's (or every worker of a range
 * j > 0 with PVAC_CHAIN_STAGE_INPUTS) first copies its chunk's inputs into worker-local buffers
 * (peer reads over xGMI when the devices differ); digests and counts are written to the caller's
 * arrays on X's device. ctx keeps the worker contexts of every device between calls. */
#define PVAC_CHAIN_CHECK_GSUM 0x100u
#define PVAC_CHAIN_STAGE_INPUTS 0x200u   /* ranges j > 0 stage their chunks even on X's device (tests) */
#define PVAC_CHAIN_IMG_BATCH2 0x400u     /* image -> records conversions in launches of 2 pairs (tests) */
#define PVAC_CHAIN_DRBG 0x800u           /* default nonces / salts from the workers' CTR_DRBGs, not splitmix */
#define PVAC_CHAIN_MAX_DEVICES 64
typedef int (*pvac_chain_step_fn)(void* user, uint32_t step, uint64_t first_input, const pvac_ct_batch* A,
                                  const pvac_ct_batch* X, const pvac_ct_batch* C, uint64_t* dev_words,
                                  uint64_t n_words, void* stream);
#define PVAC_CHAIN_MAX_DEPTH 32
typedef struct pvac_chain_opts {
    uint32_t depth;        /* 1 .. PVAC_CHAIN_MAX_DEPTH */
    uint32_t streams;      /* worker streams, 0 = 4 */
    uint64_t chunk;        /* inputs per chunk, 0 = 1024 */
    uint64_t nonce_seed;
    uint32_t flags;        /* PVAC_MUL_ORDER_CANONICAL | PVAC_MUL_WITH_SIGMA | PVAC_CHAIN_CHECK_GSUM |
                              PVAC_CHAIN_STAGE_INPUTS | PVAC_CHAIN_DRBG */
    uint32_t pad;
    uint64_t digest_n;     /* leading inputs whose final digests are written */
    uint64_t* digest_out;  /* DEVICE [digest_n], nullable */
    uint64_t count_n;      /* leading inputs whose final edge counts are written */
    uint64_t* count_out;   /* DEVICE [count_n], nullable */
    int (*fill_nonces)(void* user, uint32_t step, uint64_t first_input, uint64_t n_words, uint64_t* dev_words,
                       void* stream);
    int (*on_chunk)(void* user, uint64_t first_input, const pvac_ct_batch* C, void* stream);
    void* user;
    pvac_chain_step_fn nonces_at;    /* step hooks (above), nullable */
    pvac_chain_step_fn after_step;
    pvac_chain_step_fn salts_at;
    const int* devices;              /* HOST [n_devices] GPU ordinals; null / 0 = ctx's device */
    uint32_t n_devices;              /* 0 .. PVAC_CHAIN_MAX_DEVICES */
    uint32_t pad2;
    uint64_t* sumdigest_out;         /* DEVICE [sumdigest_n], nullable: pvac_hip_batch_sumdigest of c_depth */
    uint64_t sumdigest_n;            /* leading inputs whose sum digests are written (reads their whole c_depth) */
    /* Per-step operands (nullable): HOST [n_operands] batch descriptors of DEVICE arrays on X's device,
     * each of X->n ciphers. Step d (from 0) computes c_{d+1} = ct_mul(c_d, operands[d]) for d <
     * n_operands and ct_mul(c_d, x) after that, so the reference's own loop
     *   chain = enc_value(pk, sk, 2); for i in 1..N-1: chain = ct_mul(pk, chain, enc_value(pk, sk, 2))
     * (tests/test_main.cpp:289-293) is X = the first encryptions and operands = the later ones. The
     * step hooks' X argument is the step's operand. n_operands <= depth. */
    const pvac_ct_batch* operands;
    uint32_t n_operands;
    uint32_t pad3;
} pvac_chain_opts;
typedef struct pvac_chain_stats {
    uint64_t pair_steps;                        /* inputs x depth */
    uint64_t edges[PVAC_CHAIN_MAX_DEPTH];       /* sum over inputs of |c_k.E|, step k = index + 1 */
    uint64_t products[PVAC_CHAIN_MAX_DEPTH];    /* sum over inputs of |c_{k-1}.E| |x.E| */
    uint64_t gsum_pairs;                        /* pair-steps checked (PVAC_CHAIN_CHECK_GSUM) */
    uint64_t gsum_failed;                       /* pair-steps whose invariant failed */
    uint64_t redo;                              /* pairs re-run on the general path (ct_mul_exec) */
    uint64_t chunks;
    double seconds;                             /* wall time of the call */
    uint64_t image_steps;                       /* pair-steps whose C went to the next step as a dense
                                                   image (intermediate steps, no after_step hook or
                                                   gsum check): the layout the next step reads back */
} pvac_chain_stats;
int pvac_hip_ct_mul_chain(pvac_hip_ctx* ctx, const pvac_ct_batch* X, const pvac_chain_opts* opts,
                          pvac_chain_stats* stats);
/* Copy `bytes` between any host / device pointers (hipMemcpyDefault) ordered on `stream` (a chain
 * hook's stream, or null for the legacy stream) and wait for it: lets an FFI caller (ctypes, cgo, JNI)
 * that does not link the HIP runtime read a hook's batch view or fill its words. */
int pvac_hip_memcpy(void* dst, const void* src, size_t bytes, void* stream);
/* First input of range j of n_inputs inputs split over `parts` device ranges of whole chunks (the
 * split pvac_hip_ct_mul_chain uses): first[j] for j = 0 .. parts (first[parts] = n_inputs). */
int pvac_hip_chain_partition(uint64_t n_inputs, uint64_t chunk, uint32_t parts, uint64_t* first);

/* ct_add / ct_sub (ops/arithmetic.hpp:12-31, 43-45; combine_ciphers ops/encrypt.hpp:260-279).
 * negate_b != 0 gives ct_sub (B's weights scaled by p-1). Dense CSR output: the plan writes
 * C->l_off/e_off as exclusive scans of |A.L|+|B.L| and |A.E|+|B.E|. Sigmas are carried when
 * A, B and C all have sigma != NULL. exec: PVAC_ENOSYS when a pair has more than max(30000, the
 * context's layer limit) layers (pvac_hip_ctx_set_layer_limit); a call whose largest pair has more
 * than 30000 runs k_ct_add_deep (timing name "ct_add_deep"), its keep / remap table in global scratch. */
int pvac_hip_ct_add_plan(pvac_hip_ctx* ctx, const pvac_ct_batch* A, const pvac_ct_batch* B, pvac_ct_batch* C,
                         pvac_hip_plan* plan);
int pvac_hip_ct_add_exec(pvac_hip_ctx* ctx, const pvac_hip_plan* plan, const pvac_ct_batch* A, const pvac_ct_batch* B,
                         int negate_b, pvac_ct_batch* C);

/* ct_scale / ct_neg (ops/arithmetic.hpp:33-41): in-place w <- w * s over every edge of the
 * batch (s host scalar). */
int pvac_hip_ct_scale(pvac_hip_ctx* ctx, pvac_ct_batch* X, uint64_t s_lo, uint64_t s_hi);

/* ct_lincomb: segmented sums of optionally scaled ciphers of one resident batch, bit-exact with the
 * reference's own fold. Output i, over terms k = seg_off[i] .. seg_off[i + 1] - 1:
 *     acc = Cipher{};
 *     for k: t = X[term[k]];
 *            if (flags[k] & PVAC_TERM_SCALE) t = ct_scale(pk, t, scale[k]);   (arithmetic.hpp:33-37)
 *            acc = ct_add(pk, acc, t);                       (:12-31, guard_budget + compact_layers)
 *     C[i] = acc;
 * An empty segment gives the empty cipher; a one-term segment gives ct_add({}, t), so its unused layers
 * are dropped. An unscaled term keeps its weight words raw (non-canonical words included); a scaled
 * one goes through fp_mul whatever the scale (0 keeps its zero-weight edges, a word >= p is used as
 * given, p - 1 is ct_neg). A cipher may be a term any number of times. Sigma rows are carried when X
 * and C both have sigma, with equal sigma_words (PVAC_EINVAL when they differ). C's arrays are not X's.
 * plan: writes C->l_off / C->e_off as exclusive scans of the segments' sums of |X[term].L| and
 * |X[term].E| (dense CSR capacities; a result is never larger), fills *plan (kind 6, n_small / n_large
 * = segments on the one-pass / fold route) and synchronises once, twice when a term takes the
 * workgroup route, three times when one takes the deep-term route (below). Before anything is written
 * to C: PVAC_EINVAL for seg_off[0] != 0, a decreasing seg_off, seg_off[n] != n_terms or a term index
 * >= X->n (checked on the device, reported with the plan's statistics); PVAC_ENOSYS for a term above
 * max(30000, the context's layer limit) layers (pvac_hip_ct_add_exec's limit), a fold-route segment
 * above as many layers in all, or a term's or segment's layer or edge count >= 2^31.
 * exec: writes the rows and exact C->l_cnt / C->e_cnt. It takes this context's latest plan only, with
 * the X and S it was planned for.
 * Routes: per term, one pass over its layers and edge headers finds the layers compact_layers keeps
 * (a lane group and a 64-bit mask for terms of at most 64 layers and 8192 edges: the wave route; one
 * workgroup with its table in LDS above: the workgroup route; above 30000 layers, on a context whose
 * layer limit admits the term, one workgroup with its table in global scratch: the deep-term route,
 * counted by pvac_hip_deep_route_count). A segment within edge_budget whose terms
 * are all inside the Cipher contract (every edge's layer_id and every kept PROD parent below its own
 * |L|) is gathered in one pass: each term compacted on its own lands at its offset, which is what the
 * fold computes. Any other segment is computed by the literal loop above on pvac_hip_ct_add_plan /
 * _exec, so a lincomb plan with fold segments invalidates every earlier plan of the context, and its
 * exec the lincomb plan itself (plan again before another exec).
 * pvac_hip_ct_lincomb_path_count: since the context was created, out[0] = segments served in one pass,
 * out[1] = by the fold route, out[2] / out[3] = terms planned on the wave / workgroup route.
 * pvac_hip_ct_lincomb_status: per segment of the last exec (DEVICE, n u32, stream-ordered copy):
 * 0 = one pass, 1 = fold because over edge_budget, 2 = fold because a term is out of contract (1 wins
 * when both hold). */
#define PVAC_TERM_SCALE 0x1u
typedef struct pvac_lincomb {
    uint64_t n, n_terms;
    const uint64_t* seg_off;   /* DEVICE, n + 1, seg_off[0] = 0, non-decreasing, seg_off[n] = n_terms */
    const uint64_t* term;      /* DEVICE, n_terms indices into X */
    const uint64_t* scale;     /* DEVICE, 2 words (lo, hi) per term; NULL = no term is scaled */
    const uint32_t* flags;     /* DEVICE, per term; NULL with scale != NULL = every term is scaled */
} pvac_lincomb;
int pvac_hip_ct_lincomb_plan(pvac_hip_ctx* ctx, const pvac_ct_batch* X, const pvac_lincomb* S, pvac_ct_batch* C,
                             pvac_hip_plan* plan);
int pvac_hip_ct_lincomb_exec(pvac_hip_ctx* ctx, const pvac_hip_plan* plan, const pvac_ct_batch* X, const pvac_lincomb* S,
                             pvac_ct_batch* C);
int pvac_hip_ct_lincomb_path_count(pvac_hip_ctx* ctx, uint64_t out[4]);
int pvac_hip_ct_lincomb_status(pvac_hip_ctx* ctx, uint32_t* out, size_t n);

/* sigma_from_H for every edge of a batch (crypto/matrix.hpp:267-303): sigma of edge slot e
 * from its layer's (ztag, nonce), idx, ch and salts[e]. Requires H (set_H / gen_H). */
int pvac_hip_sigma_batch(pvac_hip_ctx* ctx, pvac_ct_batch* X, const uint64_t* salts);

/* ---------------------------------------------------------------- ct_recrypt and its parts
 * pk.ubk.inv (gen_ubk_public, crypto/matrix.hpp:95-164; core/types.hpp:81-84) from HOST memory.
 * PVAC_EINVAL unless inv is a permutation of [0, m_bits) and m_bits is the context's. Synchronous. */
int pvac_hip_ctx_set_ubk(pvac_hip_ctx* ctx, const int32_t* inv_host, uint32_t m_bits);
/* sigma_density's numerator (ops/encrypt.hpp:29-37): ones[i] (DEVICE, n u64) = sum of popcnt over
 * the ceil(m_bits / 64) words of cipher i's e_cnt[i] sigma rows; the density is
 * ones / (e_cnt * m_bits), computed by the caller (the reference divides in long double). */
int pvac_hip_sigma_popcount(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint64_t* ones);
/* ubk_apply (crypto/matrix.hpp:167-188, 306-310), in place on every sigma row:
 * out[inv[src]] = in[src] for src < m_bits. active (DEVICE, n u32, nullable): a cipher with
 * active[i] == 0 is left untouched. Needs set_ubk. */
int pvac_hip_ubk_apply(pvac_hip_ctx* ctx, pvac_ct_batch* X, const uint32_t* active);
/* compact_edges then compact_layers (ops/encrypt.hpp:39-104) of every cipher of X into C (C's arrays
 * are not X's). The plan writes C->l_off / C->e_off as exclusive scans of X's counts (the output is
 * never larger) and fills *plan (kind 5; synchronises once); the caller allocates C's rows and sigma
 * (total_layer_slots / total_edge_slots), exec writes the rows and C->l_cnt / C->e_cnt. Edges of one
 * (layer, idx, ch) are merged: the weight is the sequential fp_add chain from 0 in edge order
 * (non-canonical addends included, field.hpp:53-55), the sigma their XOR; a group is dropped only
 * when both are zero; the output is sorted by (layer, idx, P before M). An edge whose layer or idx is
 * out of range (undefined in the reference) is dropped. X and C must carry sigma (PVAC_EINVAL).
 * A cipher whose key space |L| * 2B is at most 14336 cells (21 layers at B = 337), with at most
 * 1024 layers and 65536 edges, is served by one workgroup of a batched kernel; any other by the
 * per-cipher merge path of ct_add's guard_budget. plan: PVAC_ENOSYS for a cipher of the merge path
 * with more than max(30000, the context's layer limit) layers, 2^31 edges or more, or |L| * 2B >= 2^32
 * - 1 keys. exec takes this context's latest plan only. */
int pvac_hip_compact_plan(pvac_hip_ctx* ctx, const pvac_ct_batch* X, pvac_ct_batch* C, pvac_hip_plan* plan);
int pvac_hip_compact_exec(pvac_hip_ctx* ctx, const pvac_hip_plan* plan, const pvac_ct_batch* X, pvac_ct_batch* C);
/* Ciphers compacted since the context was created (compact_exec and ct_recrypt_exec): out[0] by the
 * batched kernel, out[1] by the merge path. */
int pvac_hip_compact_path_count(pvac_hip_ctx* ctx, uint64_t out[2]);
/* ct_recrypt (ops/recrypt.hpp:26-41) of every cipher of X against the zero pool `pool`
 * (ek.zero_pool as a batch; pool->n = 0 is the empty pool). The plan writes C->l_off / C->e_off for
 * per-cipher capacities |X.L| + 8 max|pool.L| and |X.E| + 8 max|pool.E|, zeroes C->l_cnt / C->e_cnt
 * when given, and fills *plan (kind 4; max_layers / max_nb hold the pool's largest layer and edge
 * counts, and exec rejects a larger pool; synchronises once). exec, per cipher: up to 8 times, while
 * its sigma density lies outside [0.495, 0.505] (decided on the host from the exact popcounts with
 * the reference's long double expression), ct_add the pool member picks[8 i + it] % pool->n
 * (pvac_hip_ct_add_plan / _exec, guard_budget and the max(30000, layer limit) bound of a sum
 * included), then ubk_apply; at the end compact_edges
 * and compact_layers, always. picks (HOST, 8 n words) replace the loop's csprng_u64 draws
 * (recrypt.hpp:32): only the iterations that run consume theirs, in order. iters (HOST, n u32,
 * nullable) receives the iteration counts. An empty pool or e_cnt[i] == 0 copies cipher i verbatim,
 * uncompacted (recrypt.hpp:27). Needs set_ubk and sigma on X, pool and C (PVAC_EINVAL), all of one
 * even sigma_words. Intermediate results live in buffers the context owns. Synchronous. */
int pvac_hip_ct_recrypt_plan(pvac_hip_ctx* ctx, const pvac_ct_batch* X, const pvac_ct_batch* pool, pvac_ct_batch* C,
                             pvac_hip_plan* plan);
int pvac_hip_ct_recrypt_exec(pvac_hip_ctx* ctx, const pvac_hip_plan* plan, const pvac_ct_batch* X,
                             const pvac_ct_batch* pool, const uint64_t* picks, pvac_ct_batch* C, uint32_t* iters);

/* ---------------------------------------------------------------- commitments
 * commit_ct (ops/commit.hpp:12-88) of every cipher of X: digests[32 i ..] (DEVICE, 32 * X->n bytes) =
 * SHA-256("pvac.dom.commit" | H_digest | le64 canon_tag | layers | edges), a layer as u8 rule then
 * le64 ztag, nonce_lo, nonce_hi (BASE) or le64 pa, pb (any other rule), an edge as le64 layer_id,
 * le64 idx, u8 ch, le64 w_lo, le64 (w_hi & 2^63 - 1) and, when X->sigma is set, the first
 * (m_bits + 7) / 8 bytes of its sigma row (row stride X->sigma_words). X->sigma == NULL hashes no
 * sigma bytes: the commitment of the same ciphers with every edge's nbits = 0 (the fixtures'
 * "commit_weights"). H_digest is the context's (gen_H, set_H or set_H_digest; PVAC_EINVAL while it
 * is unknown) and canon_tag its params'; sigma_words * 64 < m_bits is PVAC_EINVAL. Capacity-padded
 * CSR (a ct_mul_exec output), empty ciphers and n = 0 are fine. One cipher per lane, the ciphers
 * dealt to lanes from a counter, so a ragged batch costs no more than its share of the work; one
 * very large cipher is a serial chain of its 64-byte blocks. Enqueued on the
 * context's stream; not synchronous. */
int pvac_hip_commit_ct(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint8_t* digests);

/* ---------------------------------------------------------------- metrics (utils/metrics.hpp)
 * The per-cipher readers of sigma and weights, computed where the ciphers are.
 *
 * pvac_hip_sigma_bytehist: hist (DEVICE, 256 * X->n u64): hist[256 i + b] = the number of bytes equal
 * to b among the 8 mw bytes of each of cipher i's sigma rows e_off[i] .. e_off[i] + e_cnt[i] - 1,
 * mw = ceil(m_bits / 64): a row contributes its first mw words (every byte of them, the bits past
 * m_bits in the last word included), the row stride is X->sigma_words. All 256 entries of every cipher
 * are written (an empty cipher gets zeros; the caller zeroes nothing); slots past e_cnt of a
 * capacity-padded batch are never read; n = 0 launches nothing. PVAC_EINVAL when X->sigma is null with
 * n > 0 or sigma_words * 64 < m_bits (pvac_hip_sigma_popcount's rules). Enqueued on the context's
 * stream; not synchronous. Timing label "sigma_bytehist".
 * Relation to the reference: sigma_shannon(C) (metrics.hpp:43-68) = - sum over b = 0 .. 255 with
 * freq[b] > 0 of p_b log2 p_b, p_b = (double)freq[b] / total, freq = hist's row of C and total its
 * sum. The reference counts in int, so it is undefined from 2^31 bytes per cipher (2,097,152 rows of
 * 1 KiB); the counts here are exact u64 at any size. The logarithms stay on the host (256 per cipher,
 * in the reference's floating-point order: pvac_hip.hpp's sigma_shannon).
 * Identities: sum over b of hist[256 i + b] = 8 mw e_cnt[i], and sum over b of popcount(b)
 * hist[256 i + b] = ones[i] of pvac_hip_sigma_popcount.
 *
 * pvac_hip_layer_gsum: gsum (DEVICE, 2 words (lo, hi) per layer SLOT of X, parallel to X->layers like
 * pvac_hip_base_R's output): for l < l_cnt[i], slot l_off[i] + l receives agg_layer_gsum(pk, X_i, l)
 * (metrics.hpp:70-86) = the sum over X_i's edges of layer l of +/- fp_mul(w, powg_B[idx]), + for SGN_P;
 * other slots are not written. An edge whose layer_id >= l_cnt[i] is ignored (the reference's loop
 * never asks for it). status (DEVICE, n u32, nullable), written for every cipher: 0 ok; 2 an edge of
 * that cipher has idx >= B (the reference reads past powg_B): its sums are unspecified, every write
 * stays in bounds and its neighbours are unaffected. Needs pvac_hip_ctx_set_powg (PVAC_EINVAL
 * without, as pvac_hip_check_mul_gsum). Contract (that of pvac_hip_check_mul_gsum's sums): each term
 * is the bit-exact fp_mul; the result is the exact residue mod p of the signed sum of the terms, which
 * equals the reference's fp_add / fp_sub chain whenever the terms are canonical (every cipher inside
 * the Cipher contract). There is no edge-count limit: a cipher of 2^21 edges or more (where the
 * checker's 43/42/42-bit limb sums could pass 2^64) is summed in pieces of 2^20 edges, each folded
 * mod p before the pieces are combined. PVAC_ENOSYS for a cipher of 2^28 layers or more. Synchronises
 * once (the size pass that picks the launch's LDS and scratch), then the kernel is enqueued. Timing
 * label "layer_gsum".
 * Routes, per cipher: at most 16 layers and 4096 edges: one wave of a workgroup that serves four
 * consecutive ciphers (the wave route); up to 3200 layers (48 bytes of table per layer in LDS) and
 * fewer than 2^21 edges: one workgroup (the workgroup route); 2^21 edges or more (pieces) or more
 * layers than LDS holds (the table in a slab of context scratch): the large route.
 *
 * pvac_hip_metrics_path_count, since the context was created: out[0] / out[1] = sigma_bytehist calls
 * (n > 0) served by the 16-byte-load path / the 8-byte path (a row stride different from mw, odd mw,
 * or a base pointer not 16-byte aligned); out[2] / out[3] / out[4] = ciphers pvac_hip_layer_gsum
 * served on the wave / workgroup / large route. */
int pvac_hip_sigma_bytehist(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint64_t* hist);
int pvac_hip_layer_gsum(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint64_t* gsum, uint32_t* status);
int pvac_hip_metrics_path_count(pvac_hip_ctx* ctx, uint64_t out[5]);

/* ---------------------------------------------------------------- synthetic inputs / checks
 * Fresh-shaped cipher generator used by bench.py (SURVEY §8(d) cfg 3 generator): per cipher
 * 2 BASE layers (random ztag/nonce), per layer `edges_per_layer` distinct (idx, ch), uniform
 * nonzero canonical weights, edges grouped by layer and Fisher-Yates shuffled within a layer.
 * Writes a dense CSR batch whose arrays the caller allocated for n*2 layers, n*2*epl edges. */
int pvac_hip_gen_fresh_batch(pvac_hip_ctx* ctx, uint64_t seed, uint32_t edges_per_layer, pvac_ct_batch* X);
/* Same generator keyed by GLOBAL cipher index first_index + i, so a shard reproduces the
 * corresponding slice of a single-GPU batch (multi-GPU acceptance: N-GPU output == 1-GPU). */
int pvac_hip_gen_fresh_batch_at(pvac_hip_ctx* ctx, uint64_t seed, uint64_t first_index, uint32_t edges_per_layer,
                                pvac_ct_batch* X);
/* Product-layer nonces for a planned ct_mul (C->l_off from pvac_hip_ct_mul_plan), keyed by
 * (seed, GLOBAL pair index first_index + i, product layer): replaces make_nonce128's draws
 * (core/types.hpp:77-79) for synthetic, shard-invariant batches. out: 2 words per C layer slot. */
int pvac_hip_fill_nonces(pvac_hip_ctx* ctx, uint64_t seed, uint64_t first_index, const pvac_ct_batch* A,
                         const pvac_ct_batch* B, const pvac_ct_batch* C, uint64_t* out);
/* splitmix64 stream fill (device): out[i] = splitmix64(seed + (i+1)*golden). A reproducible test
 * stream, predictable from the seed: not for nonces, salts or draws of ciphertext anyone keeps
 * (pvac_hip_drbg_fill below is). */
int pvac_hip_fill_random(pvac_hip_ctx* ctx, uint64_t seed, uint64_t* out, size_t n);

/* ---------------------------------------------------------------- device CSPRNG
 * Every context owns an SP 800-90A rev. 1 CTR_DRBG (AES-256, no derivation function, no prediction
 * resistance, seedlen 48; csrc/drbg.hpp states the construction). Its state (K, V) lives on the
 * host; a fill expands K's round keys on the host, hands the keystream AES_K(V + 1 ..) to one kernel
 * launch on the context's stream and advances the state before it returns, so two fills enqueued
 * back to back never share a counter. Word 2j of a fill is load_le64 of keystream block j's bytes
 * 0..7, word 2j + 1 of its bytes 8..15 (the reference's csprng_u64 over the concatenated bytes,
 * core/random.hpp); an odd request drops the last 8 bytes. One deviation from 90A: no 2^16-byte cap
 * per request, a fill is one generate call whatever its size.
 * pvac_hip_drbg_seed instantiates the generator from 48 bytes (NULL: 48 bytes of getrandom(2)). A
 * context never seeded seeds itself from getrandom at its first fill. A self-seeded generator
 * reseeds from getrandom after every 2^16 generate calls; an explicitly seeded one never reseeds on
 * its own, so its stream is reproducible. pvac_hip_drbg_reseed mixes 48 bytes in (NULL: getrandom).
 * A getrandom failure is PVAC_EDEVICE. pvac_hip_drbg_fill: n_words DEVICE words at out (8-byte
 * aligned), stream-ordered, not synchronous; n_words = 0 does nothing and is not counted;
 * PVAC_EINVAL for a null out with n_words > 0. Timing label "aes256_ctr".
 * pvac_hip_drbg_counts: out[0] generate calls, out[1] keystream blocks, out[2] reseeds since the
 * generator was seeded, out[3] = 1 when it seeded itself.
 * pvac_hip_aes256_ctr is the kernel alone (tests and diagnostics, like pvac_hip_fill_random): the
 * keystream AES_key(ctr + j), j = 0.., ctr a 128-bit big-endian integer (all 16 bytes count, mod 2^128).
 * The round keys travel in the kernel's arguments; the library writes no key to a device buffer.
 * pvac_hip_drbg_tile (host only): out[0] = keystream blocks one workgroup pass covers, out[1] = the
 * most workgroups a launch uses (a persistent grid strides over the tiles beyond that). */
int pvac_hip_aes256_ctr(pvac_hip_ctx* ctx, const uint8_t key[32], const uint8_t ctr_be[16], uint64_t* out_dev,
                        size_t n_words);
int pvac_hip_drbg_seed(pvac_hip_ctx* ctx, const uint8_t seed[48]);
int pvac_hip_drbg_reseed(pvac_hip_ctx* ctx, const uint8_t entropy[48]);
int pvac_hip_drbg_fill(pvac_hip_ctx* ctx, uint64_t* out_dev, size_t n_words);
int pvac_hip_drbg_counts(pvac_hip_ctx* ctx, uint64_t out[4]);
int pvac_hip_drbg_tile(uint32_t out[2]);
/* Host-only: the bucket count std::unordered_map::reserve(n) picks on this libstdc++ (the
 * emit-order pin of ct_mul, ops/arithmetic.hpp:75-76). No device access. */
uint64_t pvac_hip_bucket_count(uint64_t n);
/* per-cipher FNV-1a digest over (meta, w_lo, w_hi) of its edges in order (device out[n]). */
int pvac_hip_batch_digest(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint64_t* out);
/* per-cipher position-keyed digest (device out[n]): |E| + sum over edges e of
 * m(m(m(e * 0x9E3779B97F4A7C15 ^ meta) ^ w_lo) ^ w_hi) mod 2^64, m = the splitmix64 finaliser.
 * Order-sensitive, computed in parallel (one workgroup per cipher). */
int pvac_hip_batch_sumdigest(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint64_t* out);
/* The used rows of a capacity-padded batch (a plan's output, every pair at its capacity) packed
 * back to back into dst, e.g. before copying a result to the host. dst (DEVICE arrays): counts =
 * src's, offsets = their exclusive scans, rows and, when dst->sigma is set (src must carry sigma of
 * the same sigma_words), sigma rows; dst->n is set. dst's row arrays must hold the packed rows (src's
 * row capacity always does). totals (HOST [2]) = packed layer and edge counts. No reference
 * counterpart: the reference's Ciphers are std::vectors of exact size (core/types.hpp:95-98). */
int pvac_hip_batch_pack(pvac_hip_ctx* ctx, const pvac_ct_batch* src, pvac_ct_batch* dst, uint64_t* totals);

/* ---------------------------------------------------------------- batch_gather
 * Regroups whole ciphers of resident batches on the device: output cipher k of dst is a verbatim copy of
 * cipher pick_idx[k] of srcs[pick_src[k]]: its l_cnt layer records (all 40 bytes, pad included), its e_cnt
 * edge rows (meta, w_lo, w_hi) and, when dst->sigma is set, its sigma rows. Layer ids and PROD parents are
 * cipher-relative, so nothing is rewritten. Concat, select, permute, repeat and split are all this call.
 * Sources are dense or capacity-padded CSR with any offsets; slots past a cipher's counts are never read.
 * dst comes out as dense CSR: l_cnt / e_cnt copied, l_off / e_off their exclusive scans, dst->n = m. A
 * cipher may be picked any number of times and a source may go unused. No reference counterpart (its
 * Ciphers are std::vectors a caller moves around at will).
 * Null picks: pick_src == NULL with pick_idx given requires n_src == 1, and every pick comes from srcs[0];
 * pick_idx == NULL requires pick_src == NULL and m == the sum of srcs[j].n: the output is the
 * concatenation of the sources in order, and no pick list is built.
 * Contract: dst's arrays overlap no source's (documented, not checked).
 *
 * pvac_hip_batch_gather_plan validates before anything is written to dst: PVAC_EINVAL for n_src == 0 with
 * m > 0, n_src > PVAC_GATHER_MAX_SOURCES, the null-pick rules, dst->sigma set while any source has no
 * sigma or a different sigma_words, and (found on the device, reported with the totals' read-back) a
 * pick_src[k] >= n_src or a pick_idx[k] >= srcs[pick_src[k]].n; PVAC_ENOSYS for m >= 2^31 - 1. Otherwise it
 * writes dst's four index arrays (m entries) and sets totals[0], [1] (HOST) to the layer and edge rows
 * needed. It synchronises once. The uploaded source table and the tile tables live in storage of the
 * gather's own, so a pending plan of another operation stays valid. dst's rows (and dst->sigma) are
 * allocated between plan and exec; tiles are dealt for both a weights-only copy and one with the sources'
 * common sigma width.
 *
 * pvac_hip_batch_gather_exec takes this context's latest gather plan only, for the same G (sources, picks,
 * m) and the same index arrays of dst (PVAC_EINVAL otherwise; dst->sigma is checked as by the plan).
 * PVAC_ENOMEM, with nothing written, when the plan's totals exceed layer_cap / edge_cap (the capacity
 * check pvac_hip_batch_pack lacks). m == 0 launches nothing. Enqueued on the context's stream; not
 * synchronous. Timing label "batch_gather". A plan may be executed more than once.
 *
 * Work is dealt in tiles numbered through the output: at most ept consecutive edge rows of one cipher
 * (16 KiB of meta, w_lo, w_hi and sigma words) or at most lpt consecutive layer records of one, a wave per
 * tile, four tiles in flight per workgroup, each wave taking a run of consecutive tiles, the grid capped
 * at 8 workgroups per CU. One 345 K-edge cipher spreads over the device and 2^20 small ciphers do not
 * cost a workgroup each. Edge arrays move 16 bytes per lane where a tile's source and destination
 * addresses agree mod 16 after an 8-byte head (8-byte tail for an odd end), 8 bytes where they do not;
 * sigma rows 16 bytes when sigma_words is even and dst's and every source's sigma base is 16-byte aligned,
 * 8 bytes otherwise; layer records as 8-byte words. No store lands outside the rows of the cipher copied.
 *
 * pvac_hip_batch_gather_path_count, since the context was created: out[0] / out[1] = exec calls (m > 0)
 * whose sigma rows moved 16 / 8 bytes at a time (a call without sigma counts under out[1], as in the
 * codec), out[2] = tiles dealt, out[3] = output ciphers.
 * pvac_hip_batch_gather_tile (host only, no context): out[0] = ept, out[1] = lpt for a sigma width
 * (0 = weights only). */
#define PVAC_GATHER_MAX_SOURCES 1024
typedef struct pvac_gather {
    const pvac_ct_batch* srcs;  /* HOST [n_src] descriptors of DEVICE arrays on the context's device */
    uint32_t n_src, pad;
    uint64_t m;                 /* output ciphers */
    const uint32_t* pick_src;   /* DEVICE [m], nullable */
    const uint64_t* pick_idx;   /* DEVICE [m], nullable */
} pvac_gather;
int pvac_hip_batch_gather_plan(pvac_hip_ctx* ctx, const pvac_gather* G, pvac_ct_batch* dst, uint64_t totals[2]);
int pvac_hip_batch_gather_exec(pvac_hip_ctx* ctx, const pvac_gather* G, pvac_ct_batch* dst, uint64_t layer_cap,
                               uint64_t edge_cap);
int pvac_hip_batch_gather_path_count(pvac_hip_ctx* ctx, uint64_t out[4]);
int pvac_hip_batch_gather_tile(uint32_t sigma_words, uint32_t out[2]);

/* ---------------------------------------------------------------- LPN PRF
 * SecKey (core/types.hpp:134-137): prf_k and the LPN secret (ceil(lpn_n/64) words, host) with
 * pk.prm's lpn_t and noise rate tau_num/tau_den. The PRF also needs pk.H_digest: it is taken
 * from gen_H / set_H, or given with set_H_digest. */
int pvac_hip_ctx_set_secret(pvac_hip_ctx* ctx, const uint64_t prf_k[4], const uint64_t* lpn_s_host, uint32_t lpn_n,
                            uint32_t lpn_t, uint32_t tau_num, uint32_t tau_den);
int pvac_hip_ctx_set_H_digest(pvac_hip_ctx* ctx, const uint8_t digest[32]);
/* prf over n seeds (device, 3 words per seed: {ztag, nonce_lo, nonce_hi} = pvac::RSeed):
 * kind 0..5 = prf_R_core with domain pvac.prf.r.1..3 / pvac.prf.noise.1..3 (crypto/lpn.hpp:188-261),
 * 6 = prf_R (:263-268), 7 = prf_R_noise (:270-275). out: device, 2 words (lo, hi) per seed. */
int pvac_hip_prf(pvac_hip_ctx* ctx, int kind, size_t n, const uint64_t* seeds, uint64_t* out);

/* ---------------------------------------------------------------- encryption
 * enc_value (ops/encrypt.hpp:281-287) over n plaintexts (device u64). The reference draws every
 * random choice from getrandom (csprng_u64); here value i's draws are rnd[i * rnd_stride ...], in
 * the reference's order (mask, then enc_fp_depth(-mask), then enc_fp_depth(v + mask)): with the
 * draws the reference consumed, the output is byte-identical. C: 2 layers and edges_per_value
 * edge slots per value (pvac_hip_enc_caps), l_off/l_cnt/e_off/e_cnt written by the call
 * (capacity-padded CSR). status: device u32 per value: 0 ok; 1 rnd_stride draws were not enough;
 * 2 a merged edge group cancelled exactly (probability ~1/p; not reproduced). Needs set_secret,
 * the H digest, set_powg, and H for PVAC_ENC_WITH_SIGMA. */
#define PVAC_ENC_WITH_SIGMA 0x1u
int pvac_hip_enc_caps(pvac_hip_ctx* ctx, uint32_t* layers_per_value, uint32_t* edges_per_value, uint32_t* draws_hint);
int pvac_hip_enc_value(pvac_hip_ctx* ctx, size_t n, const uint64_t* values, const uint64_t* rnd, uint32_t rnd_stride,
                       pvac_ct_batch* C, uint32_t flags, uint32_t* status);
/* enc_value_depth(pk, sk, v, depth_hint) (ops/encrypt.hpp:281-287): as pvac_hip_enc_value with the
 * noise plan of depth_hint (plan_noise, encrypt.hpp:16-27: more Z2 / Z3 groups as the hint grows;
 * supported while 8 + 2 Z2 + 3 Z3 is within the context's plan limit, pvac_hip_ctx_set_enc_plan_limit:
 * 256 by default, i.e. depth_hint <= 124 with the default Params, else PVAC_ENOSYS; above 256 edges the
 * values run as VALUE items of pvac_hip_enc_items on its wide route, with the same output layout;
 * the Params noise fields from pvac_hip_ctx_set_noise). values[i] = 0 gives
 * enc_zero_depth(pk, sk, depth_hint) (encrypt.hpp:293-298) byte for byte: fp_add(0, mask) is mask and
 * the draws are the same. Size outputs and rnd_stride with
 * pvac_hip_enc_caps_depth. */
int pvac_hip_enc_caps_depth(pvac_hip_ctx* ctx, int depth_hint, uint32_t* layers_per_value, uint32_t* edges_per_value,
                            uint32_t* draws_hint);
int pvac_hip_enc_value_depth(pvac_hip_ctx* ctx, size_t n, const uint64_t* values, const uint64_t* rnd, uint32_t rnd_stride,
                             int depth_hint, pvac_ct_batch* C, uint32_t flags, uint32_t* status);
/* A ragged batch of encryptions in one call: item i is a bare enc_fp_depth (one BASE layer, no mask,
 * a plaintext of two words) or the masked enc_value_depth form, with its own depth hint, hence its
 * own noise plan, and its own draw segment rnd[rnd_off .. rnd_off + rnd_cnt) of the DEVICE array rnd
 * (rnd_words words). Draws are consumed in the reference's order: an FP item as one enc_fp_depth
 * (nonce, signal picks, coefficients, salts, noise groups, shuffle); a VALUE item as mask, the -mask
 * half, the v + mask half, exactly as pvac_hip_enc_value_depth. enc_text (utils/text.hpp:39-61) is a
 * VALUE item (the length, hint 0) followed by one FP item per 15-byte block with hints 2, 3, ...
 * Segments are per item because rejection sampling makes the number of draws data-dependent.
 * items is HOST memory. pvac_hip_enc_items_caps gives the sizes: layer_slots = sum of halves (1 or 2),
 * edge_slots = sum of halves x (8 + 2 Z2 + 3 Z3), draws_hint[i] (HOST, n words, nullable) a segment
 * length that suffices unless rejections exceed its slack. pvac_hip_enc_items writes C as
 * capacity-padded CSR: l_off = prefix sums of the halves, e_off = prefix sums of the pre-merge edge
 * counts, e_cnt exact; C's index arrays hold n entries, C->layers layer_cap, the edge arrays (and
 * C->sigma with PVAC_ENC_WITH_SIGMA) edge_cap slots. status (DEVICE, n u32) as for pvac_hip_enc_value:
 * 0 ok, 1 the item's segment ran out (its rows are meaningless; its neighbours are unaffected), 2 a
 * merged group cancelled exactly. Before anything is launched or written: PVAC_EINVAL for an unknown
 * kind or a draw range outside rnd_words, PVAC_ENOSYS for a plan beyond the context's plan limit (by
 * default 256 pre-merge edges per half: depth hint > 124 with the default Params), PVAC_ENOMEM when
 * layer_cap / edge_cap are too small.
 * Needs what pvac_hip_enc_value needs. Synchronises once per sub-batch (the item records' upload); the
 * kernels are enqueued. pvac_hip_enc_value(_depth) keep their own kernels up to 256 edges. */
/* The plan limit of a context: the most pre-merge edges per half (8 + 2 Z2 + 3 Z3) an encryption may
 * plan. Every encryption entry (enc_caps_depth, enc_value_depth, enc_items_caps, enc_items) refuses a
 * plan above it with PVAC_ENOSYS before anything is launched or written. Up to 256 edges an item runs
 * the narrow kernels (k_enc.hip, k_enc_items.hip); above, the wide route (k_enc_wide.hip), which keeps
 * its per-half key tables in global scratch, is linear in the plan and gives what the reference gives
 * from the same draws. The reference has no bound: enc_text uses depth hint 2 + b for block b, so with
 * the default Params a message of 1,846 bytes or more needs hint 125 (257 edges). The default of 256
 * is kept on purpose: scratch is about 1 KB per pre-merge edge with sigma (m_bits / 8 bytes of sigma
 * row plus 54 bytes of rows, 70 on the wide route), and a text's pre-merge edges grow with the square
 * of its length (17,480 for 1,860 bytes, 975,452 for 15,000), so a caller raises the limit knowing what
 * a message costs. set: PVAC_EINVAL outside [PVAC_ENC_PLAN_LIMIT_DEFAULT, PVAC_ENC_PLAN_LIMIT_MAX].
 * A call runs in sub-batches of consecutive items, cut where their pre-merge edges would pass the
 * context's budget (default 2^22; an item above it runs alone; set: PVAC_EINVAL for 0): the scratch
 * arena is sized by the largest sub-batch, and results do not depend on the cuts. A call of narrow
 * items within the budget is one sub-batch and launches what it always did.
 * PVAC_ENC_WIDE_ALL (pvac_hip_enc_items' flags) sends every item down the wide route, whatever its
 * plan: for tests and measurements, the two routes agree on every plan both can run.
 * draws_hint of a plan above 256 edges carries a slack of max(146, ceil(6 (28 + Z2 + 3 Z3) / B)) draws
 * per half in place of 32 (derived in csrc/enc_wide.hpp: expected rejections grow with the plan).
 * pvac_hip_enc_path_count, since the context was created: out[0] / out[1] = items run by the narrow /
 * the wide route, out[2] = sub-batches, out[3] = runs (an enc_items call with n > 0, an enc_value(_depth) call). */
#define PVAC_ENC_WIDE_ALL 0x2u
#define PVAC_ENC_PLAN_LIMIT_DEFAULT 256u
#define PVAC_ENC_PLAN_LIMIT_MAX (1u << 24)
#define PVAC_ENC_BUDGET_DEFAULT (1ull << 22)
int pvac_hip_ctx_set_enc_plan_limit(pvac_hip_ctx* ctx, uint32_t max_pre_edges); /* DEFAULT..MAX, else PVAC_EINVAL */
int pvac_hip_ctx_enc_plan_limit(pvac_hip_ctx* ctx, uint32_t* out);
int pvac_hip_ctx_set_enc_budget(pvac_hip_ctx* ctx, uint64_t pre_edges);
int pvac_hip_ctx_enc_budget(pvac_hip_ctx* ctx, uint64_t* out);
int pvac_hip_enc_path_count(pvac_hip_ctx* ctx, uint64_t out[4]);
#define PVAC_ENC_ITEM_FP    0u  /* enc_fp_depth(pk, sk, Fp{v_lo, v_hi}, depth_hint), encrypt.hpp:162-258: 1 BASE layer */
#define PVAC_ENC_ITEM_VALUE 1u  /* enc_value_depth(pk, sk, v_lo, depth_hint), :281-287: 2 layers (v_lo = 0: enc_zero_depth) */
typedef struct pvac_enc_item {  /* HOST memory */
    uint64_t v_lo, v_hi;        /* passed to the equations as given, no canonicalisation (the reference does none) */
    int32_t  depth_hint;
    uint32_t kind;
    uint64_t rnd_off, rnd_cnt;  /* this item's draws: rnd[rnd_off .. rnd_off + rnd_cnt) */
} pvac_enc_item;
int pvac_hip_enc_items_caps(pvac_hip_ctx* ctx, size_t n, const pvac_enc_item* items, uint64_t* layer_slots,
                            uint64_t* edge_slots, uint64_t* draws_hint);
int pvac_hip_enc_items(pvac_hip_ctx* ctx, size_t n, const pvac_enc_item* items, const uint64_t* rnd, uint64_t rnd_words,
                       pvac_ct_batch* C, uint64_t layer_cap, uint64_t edge_cap, uint32_t flags, uint32_t* status);

/* Text packing (utils/text.hpp:15-37, 63-87), HOST memory, no context. pvac_text_pack: block b of msg
 * (up to 15 bytes, little-endian) as fp_from_words(lo, hi) into v_out[2 b], v_out[2 b + 1];
 * *blocks = ceil(len / 15); PVAC_ENOMEM (with *blocks set) when block_cap is smaller. pvac_text_unpack:
 * dec holds 2 words per cipher of one message, cipher 0 the length; out receives
 * min(length, 15 (n_ciphers - 1)) bytes and *len that count; *flags bit 0: the length's high word was
 * not 0 (the reference warns and goes on), bit 1: the length was clipped to the blocks present.
 * n_ciphers = 0 is the empty message. PVAC_ENOMEM (with *len set) when cap is smaller. */
#define PVAC_TEXT_LEN_HI 0x1u
#define PVAC_TEXT_LEN_CLIPPED 0x2u
int pvac_text_pack(const uint8_t* msg, size_t len, uint64_t* v_out, size_t block_cap, size_t* blocks);
int pvac_text_unpack(const uint64_t* dec, size_t n_ciphers, uint8_t* out, size_t cap, size_t* len, uint32_t* flags);

/* prf_R of every BASE layer of X (ops/decrypt.hpp:44-46): R_out device, 2 words per layer SLOT
 * (slots addressed by l_off/l_cnt; PROD slots get 0) — the R_base input of pvac_hip_dec_value. */
int pvac_hip_base_R(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint64_t* R_out);

/* ---------------------------------------------------------------- decryption
 * dec_value (ops/decrypt.hpp:12-89) over a batch, given the BASE-layer R values (prf_R of each
 * BASE layer's seed under the secret key, crypto/lpn.hpp): R of every other layer is the product
 * of its parents' (layer_R_cached), inverses are fp_inv (field.hpp:229-273), and
 * dec = sum(+/- w * powg_B[idx] * R[layer]^-1), + for SGN_P. Bit-identical to the reference.
 * set_powg: pk.powg_B as `count` >= B (lo, hi) pairs in HOST memory.
 * R_base: device, 2 words per layer SLOT of X (parallel to X->layers; read for BASE layers only).
 * out: device, 2 words (lo, hi) per cipher. status: device u32 per cipher: 0 ok; 1 the layer
 * graph has a cycle or an out-of-range parent (the reference aborts); 2 an edge references a
 * layer or idx out of range (out-of-bounds reads in the reference). out is undefined unless 0. */
int pvac_hip_ctx_set_powg(pvac_hip_ctx* ctx, const uint64_t* powg_host, uint32_t count);
int pvac_hip_dec_value(pvac_hip_ctx* ctx, const pvac_ct_batch* X, const uint64_t* R_base, uint64_t* out,
                       uint32_t* status);

/* ---------------------------------------------------------------- .ct codec (host memory)
 * The reference's ciphertext file format (tests/add.cpp:22-155: saveCts / loadCts, putLayer,
 * putEdge) <-> SoA batches in HOST memory; no context or device needed (copy to the device with
 * hipMemcpy, or parse straight into pinned buffers). PROD layers carry no seed on disk, so parsed
 * PROD layers have ztag = nonce = 0. Every edge of a file must carry the same sigma nbits. */
#define PVAC_CT_MIXED_SIGMA 0x1u   /* pvac_ct_file_info.flags: edges disagree on sigma nbits */
typedef struct pvac_ct_file_info {
    uint64_t n_ciphers, total_layers, total_edges;
    uint32_t sigma_bits;    /* nbits of every edge's sigma (0: the file carries no sigmas) */
    uint32_t sigma_words;   /* ceil(sigma_bits / 64) */
    uint32_t flags;
    uint32_t pad;
} pvac_ct_file_info;
/* Validate a file image and size it (PVAC_EINVAL on a malformed or truncated image). */
int pvac_ct_scan(const uint8_t* buf, size_t len, pvac_ct_file_info* info);
/* Decode into X (host arrays sized from pvac_ct_scan; X->n = n_ciphers; X->sigma nullable, else
 * X->sigma_words >= info.sigma_words). Writes dense CSR l_off/l_cnt/e_off/e_cnt. threads <= 0:
 * one per hardware thread. PVAC_ENOSYS if edges disagree on sigma nbits. */
int pvac_ct_parse(const uint8_t* buf, size_t len, pvac_ct_batch* X, int threads);
/* Bytes pvac_ct_write produces for X; sigma_bits is written per edge when X->sigma != NULL
 * (the reference writes m_bits = 8192), 0 otherwise. */
int pvac_ct_serialized_size(const pvac_ct_batch* X, uint32_t sigma_bits, uint64_t* bytes);
int pvac_ct_write(const pvac_ct_batch* X, uint32_t sigma_bits, uint8_t* out, size_t capacity, uint64_t* written,
                  int threads);

/* ---------------------------------------------------------------- .ct codec (device memory)
 * The same format where the ciphers are: a resident batch becomes a byte-exact .ct file image in device
 * memory (one copy to pinned memory and one write() finish a save), and an uploaded image becomes a
 * resident batch. The host codec above is the specification: the image is exactly pvac_ct_write's
 * bytes, the parsed arrays exactly pvac_ct_parse's. File I/O stays with the caller.
 *
 * pvac_ct_index (host, no context): pvac_ct_scan plus the byte offset of every cipher's |L| field:
 * pos (HOST, n_ciphers + 1 words), pos[0] = 16, pos[n] = len. Same validation and codes as pvac_ct_scan;
 * PVAC_ENOMEM (with *info filled) when pos_cap < n_ciphers + 1. A file whose edges disagree on nbits is
 * flagged (PVAC_CT_MIXED_SIGMA) here and refused by the device parser, as by the host parser.
 *
 * Image buffer: `image` (DEVICE) is 16-byte aligned (PVAC_EINVAL otherwise) and its allocation holds
 * (cap + 15) & ~15 bytes for a write, (len + 15) & ~15 bytes for a parse: the kernels move aligned
 * 16-byte granules. The writer changes no byte at or after pos[n]; the parser reads no byte at or after
 * the rounded length.
 *
 * pvac_hip_ct_image_plan: the sizes of X's image. nbits = X->sigma ? sigma_bits : 0
 * (pvac_ct_serialized_size's rule). pos (DEVICE, X->n + 1 words) as above, *bytes (HOST) = pos[n].
 * Dense or capacity-padded CSR (a ct_mul_exec output); slots past the counts are never read.
 * PVAC_EINVAL when X->sigma is set and ceil(sigma_bits / 64) > X->sigma_words, and (with *bytes set) for a
 * layer whose rule >= 256: the host writer sizes such a layer by the u32 and writes its low byte, so
 * its output is not a file. PVAC_ENOSYS for sigma_bits above 130816 (an edge record beyond a 16 KiB
 * tile), sigma_words above 4096 or 2^31 - 1 ciphers or more. Synchronises once.
 *
 * pvac_hip_ct_image_write: image[0, pos[n]) = exactly the bytes pvac_ct_write produces for X's used rows:
 * a rule other than 0 or 1 writes its byte and 24 zero bytes, PROD writes pa, pb only, n = 0 gives the
 * 16-byte header, sigma words are copied whole (nw = ceil(nbits / 64) words per row with row stride
 * sigma_words, bits past nbits included). It takes this context's latest image plan only: the pos that
 * plan filled, for the same X and sigma_bits (PVAC_EINVAL otherwise). PVAC_ERANGE when pos[n] > cap
 * (pvac_ct_write's code). Enqueued on the context's stream; not synchronous. Timing label "ct_image_write".
 *
 * pvac_hip_ct_image_parse: image (DEVICE, the len bytes of a .ct file) with pos (DEVICE, n + 1 words: the
 * caller uploads pvac_ct_index's) -> X as dense CSR, exactly the arrays pvac_ct_parse produces: l_off /
 * e_off are exclusive scans of the counts read from the image, X->n is set; layer records are written in
 * full (40 bytes: PROD has ztag = nonce = 0, an unknown rule is kept with everything else 0, pad = 0);
 * sigma words from nw up to X->sigma_words are zeroed; X->sigma == NULL skips sigma. X's index arrays
 * hold n entries, X->layers layer_cap slots, the edge arrays (and X->sigma) edge_cap slots. Every edge
 * of the image carries nbits = sigma_bits (pvac_ct_file_info.sigma_bits).
 * Validation comes before any row is written, from pos, len and the two count words of each cipher alone:
 * pos non-decreasing, pos[0] == 16, pos[n] == len, 8 + |E| eb <= pos[i + 1] - pos[i] with
 * eb = 28 + 8 nw, and the walk of |L| layer records from pos[i] + 8 ending exactly at
 * pos[i + 1] - |E| eb. status (DEVICE, n u32, nullable): 0 ok, 1 the cipher fails one of these. Any
 * status 1 returns PVAC_EINVAL, totals above layer_cap or edge_cap PVAC_ENOMEM, both with nothing
 * written to X. An edge whose nbits field differs from sigma_bits gives its cipher status 2 and the call
 * PVAC_EINVAL; X's rows are unspecified then (every write stays in bounds). The 16 header bytes are not
 * checked beyond pos[0]: pvac_ct_index did. PVAC_ENOSYS as for the plan. Synchronises once, at its end:
 * the row kernels take the validation's verdict on the device. Timing label "ct_image_parse".
 *
 * Work is dealt in tiles of whole edge records (at most 16 KiB of image) numbered through the batch, so
 * one cipher of 345 K edges and 2^20 small ones both fill the device. Sigma rows move 16 bytes at a
 * time when nw and sigma_words are even and X->sigma is 16-byte aligned, 8 bytes at a time otherwise.
 * pvac_hip_ct_image_path_count, since the context was created: out[0] / out[1] = writes served by the
 * 16-byte / the 8-byte sigma path, out[2] / out[3] the same for parses; a weights-only call (no sigma,
 * or sigma_bits = 0 on a write) counts under the 8-byte path. */
int pvac_ct_index(const uint8_t* buf, size_t len, pvac_ct_file_info* info, uint64_t* pos, size_t pos_cap);
int pvac_hip_ct_image_plan(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint32_t sigma_bits, uint64_t* pos, uint64_t* bytes);
int pvac_hip_ct_image_write(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint32_t sigma_bits, const uint64_t* pos,
                            uint8_t* image, uint64_t cap);
int pvac_hip_ct_image_parse(pvac_hip_ctx* ctx, const uint8_t* image, uint64_t len, const uint64_t* pos, uint64_t n,
                            uint32_t sigma_bits, pvac_ct_batch* X, uint64_t layer_cap, uint64_t edge_cap,
                            uint32_t* status);
int pvac_hip_ct_image_path_count(pvac_hip_ctx* ctx, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* PVAC_HIP_H */
