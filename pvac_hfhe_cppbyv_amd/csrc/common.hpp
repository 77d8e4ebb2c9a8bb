// common.hpp — shared device helpers and launch declarations for libpvac_hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pvac_hip.h"
#include "deep_ops.hpp"
#include "fp127.hpp"
#include "gather_tiles.hpp"

namespace pvhip {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ULL;   // ct_mul key hash (ops/arithmetic.hpp:73)

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint32_t meta_layer(uint64_t m) { return (uint32_t)m; }
__device__ __forceinline__ uint32_t meta_idx(uint64_t m) { return (uint32_t)(m >> 32) & 0xFFFFu; }
__device__ __forceinline__ uint32_t meta_ch(uint64_t m) { return (uint32_t)(m >> 48) & 0xFFu; }
__device__ __forceinline__ uint64_t make_meta(uint32_t layer, uint32_t idx, uint32_t ch) {
    return (uint64_t)layer | ((uint64_t)(idx & 0xFFFFu) << 32) | ((uint64_t)(ch & 0xFFu) << 48);
}

// Wave64 inclusive prefix sum with DPP (row_shr 1/2/4/8 inside 16-lane rows, then row_bcast
// 15/31 across rows): six VALU ops, no LDS round trips (unlike __shfl_up's ds_bpermute).
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t x) {
    x += __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += __builtin_amdgcn_update_dpp(0u, x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0u, x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0u, x, 0x118, 0xf, 0xf, false);   // row_shr:8
    x += __builtin_amdgcn_update_dpp(0u, x, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0u, x, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return x;
}

// OR over the 64 lanes of a wave (same DPP network; lane 63 ends with the total), uniform result
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t x) {
    x |= __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xf, 0xf, false);
    x |= __builtin_amdgcn_update_dpp(0u, x, 0x112, 0xf, 0xf, false);
    x |= __builtin_amdgcn_update_dpp(0u, x, 0x114, 0xf, 0xf, false);
    x |= __builtin_amdgcn_update_dpp(0u, x, 0x118, 0xf, 0xf, false);
    x |= __builtin_amdgcn_update_dpp(0u, x, 0x142, 0xa, 0xf, false);
    x |= __builtin_amdgcn_update_dpp(0u, x, 0x143, 0xc, 0xf, false);
    return __builtin_amdgcn_readlane(x, 63);
}

__device__ __forceinline__ uint64_t wave_or_u64(uint64_t v) {
    return (uint64_t)wave_or_u32((uint32_t)v) | ((uint64_t)wave_or_u32((uint32_t)(v >> 32)) << 32);
}

// Workgroup-wide exclusive scan of one u32 per thread. `part` is LDS scratch of BS/64 words.
template <int BS>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* part, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t x = wave_incl_scan_u32(v);
    if (lane == 63) part[wave] = x;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < BS / 64; ++w) {
        const uint32_t pw = part[w];
        base += (w < wave) ? pw : 0u;
        tot += pw;
    }
    total = tot;
    __syncthreads();
    return base + x - v;
}

// ---------------------------------------------------------------- launch wrappers
// (defined in the .hip translation units; all enqueue on `st` and return hipError_t)
hipError_t launch_fp_binop(int op, const uint64_t* alo, const uint64_t* ahi, const uint64_t* blo,
                           const uint64_t* bhi, uint64_t* clo, uint64_t* chi, size_t n, hipStream_t st);
hipError_t launch_fill_random(uint64_t seed, uint64_t* out, size_t n, hipStream_t st);
// the AES-256 counter-mode keystream of a job (aes256.hpp, k_drbg.hip): out[0, n_words), n_words <= 2 nb.
// A workgroup pass covers kDrbgTile blocks; the persistent grid has at most kDrbgGridCap workgroups.
struct aes_ctr_job;
constexpr uint32_t kDrbgTile = 1024, kDrbgGridCap = 512;
hipError_t launch_aes256_ctr(const aes_ctr_job& job, uint64_t* out, size_t n_words, hipStream_t st);
hipError_t launch_gen_fresh(uint64_t seed, uint64_t first, uint32_t epl, uint32_t B, const pvac_ct_batch& X,
                            hipStream_t st);
hipError_t launch_fill_nonces(uint64_t seed, uint64_t first, const pvac_ct_batch& A, const pvac_ct_batch& B,
                              const uint64_t* c_l_off, uint64_t* out, hipStream_t st);
hipError_t launch_batch_digest(const pvac_ct_batch& X, uint64_t* out, hipStream_t st);
hipError_t launch_batch_sumdigest(const pvac_ct_batch& X, uint64_t* out, hipStream_t st);
hipError_t launch_ct_scale(const pvac_ct_batch& X, uint64_t slo, uint64_t shi, hipStream_t st);

// x mod d for a runtime divisor d < 2^32 without a 64-bit division: m = floor((2^64-1)/d),
// q = mulhi(x, m) undershoots floor(x/d) by at most 2, so two conditional subtracts finish.
struct fastmod64 {
    uint64_t d, m;
};
__host__ __device__ inline fastmod64 make_fastmod64(uint64_t d) { return fastmod64{d, d ? ~0ull / d : 0}; }
__device__ __forceinline__ uint64_t fmod64(uint64_t x, const fastmod64& f) {
    const uint64_t q = __umul64hi(x, f.m);
    uint64_t r = x - q * f.d;
    r = r >= f.d ? r - f.d : r;
    r = r >= f.d ? r - f.d : r;
    return r;
}

// plan statistics written by the plan kernels (device, zeroed before launch)
struct plan_stats {
    unsigned long long total_layers, total_edges;   // the plan scans' totals (pvac_hip_ctx::totals)
    unsigned long long n_small, n_large, n_invalid;
    unsigned int max_keys, max_prod, max_na, max_nb, max_buckets, max_layers;
};

// pair classes written by the mul plan
enum : uint8_t { PAIR_EMPTY = 0, PAIR_SMALL = 1, PAIR_LARGE = 2 };

hipError_t launch_plan_mul(const pvac_ct_batch& A, const pvac_ct_batch& B, pvac_ct_batch& C, uint8_t* pair_class,
                           uint64_t* large_ids, plan_stats* stats, const uint32_t* nb_table, uint32_t nb_table_len,
                           uint32_t Bm, hipStream_t st);
hipError_t launch_gather_large(const pvac_ct_batch& A, const pvac_ct_batch& B, const uint64_t* ids, uint64_t n,
                               uint64_t* out, hipStream_t st);
hipError_t launch_plan_add(const pvac_ct_batch& A, const pvac_ct_batch& B, pvac_ct_batch& C, plan_stats* stats,
                           uint8_t* pair_class, uint64_t* merge_ids, uint64_t edge_budget, hipStream_t st);
hipError_t launch_gather_merge(const pvac_ct_batch& A, const pvac_ct_batch& B, const pvac_ct_batch& C,
                               const uint64_t* ids, uint64_t n, uint64_t* out, hipStream_t st);
// in-place exclusive scan of n u64 values (or of two arrays of n values at once: one launch per
// scan kernel); scratch >= scan_scratch_words(n) u64
size_t scan_scratch_words(size_t n);
hipError_t launch_exclusive_scan2_u64(uint64_t* d0, uint64_t* d1, size_t n, uint64_t* scratch,
                                      unsigned long long* total0, unsigned long long* total1, hipStream_t st);
hipError_t launch_exclusive_scan_u64(uint64_t* data, size_t n, uint64_t* scratch, unsigned long long* total_out,
                                     hipStream_t st);

// ---- ct_mul, fresh-shape path (k_mul_fresh.hip): LDS-resident, one workgroup per pair
constexpr uint32_t kFreshKeysMax = 1536;    // |A.L||B.L|B key slots
constexpr uint32_t kFreshProdMax = 4096;    // |A.E||B.E| products
constexpr uint32_t kFreshEdgesMax = 256;    // |A.E|, |B.E|
constexpr uint32_t kFreshLayersMax = 64;    // |C.L| before compaction

// One 64-byte header record per pair (written by k_mul_layers_fresh, read by k_ct_mul_fresh with
// a single scalar load): every per-pair field the aggregation kernel needs, in one cache line.
struct __attribute__((aligned(64))) fresh_rec {
    uint64_t aeo, beo, ceo;      // edge offsets of A, B, C
    uint64_t alo, blo, clo;      // layer offsets
    uint64_t nb_magic;           // fastmod64 multiplier of nbk
    uint32_t shape;              // nA | nB << 16   (each <= kFreshEdgesMax)
    uint16_t nbk;                // libstdc++ bucket count after reserve(nA nB); 0 = not a fresh pair
    uint8_t LA, LB;
};
static_assert(sizeof(fresh_rec) == 64, "fresh_rec is one cache line");

struct mul_fresh_args {
    pvac_ct_batch A, B, C;
    fresh_rec* recs;             // per pair, filled by k_mul_layers_fresh
    const uint64_t* nonces;
    const uint8_t* pair_class;
    uint32_t* pair_status;       // 0 = reference order, 1 = canonical order, 2 = rejected (bad refs)
    const uint32_t* nb_table;    // libstdc++ bucket count after reserve(n), n <= kFreshProdMax
    const uint64_t* nb_magic;    // fastmod64 multipliers for nb_table
    uint32_t* salt_pos;          // nullable: per output edge slot, its hash-order index
    uint64_t* redo_ids;          // pairs whose key sums cancelled to 0 mod p (re-run on the general path)
    unsigned int* redo_cnt;      // their count (device, zeroed before the launch)
    uint64_t canon_tag;
    uint64_t edge_budget;
    uint32_t Bm;
    uint32_t flags;
    // launch sizing (maxima over the small pairs of the batch)
    uint32_t ks_max, prod_max, na_max, nb_max, buckets_max, layers_max;
};
// pair_status values of ct_mul (device array): 0 reference order, 1 canonical order, 2 rejected,
// 3 = the fresh kernel found a key sum of 0 mod p and left the pair to the general path
constexpr uint32_t kPairRedo = 3;
hipError_t launch_mul_layers_fresh(const mul_fresh_args& a, hipStream_t st);
// args_dev: device copy of `a` (the kernel reads its arguments from memory, see k_mul_fresh.hip)
hipError_t launch_ct_mul_fresh(const mul_fresh_args& a, const mul_fresh_args* args_dev, int num_cus, hipStream_t st);

// ---- LPN PRF (k_prf.hip): prf_R_core / prf_R / prf_R_noise (crypto/lpn.hpp:159-275)
struct prf_consts {
    uint32_t mid[8];          // SHA-256 state after block 0 of the key derivation (prf_k, canon, H_digest[0..24))
    uint64_t hd_tail;         // H_digest[24..32) as a little-endian u64
    uint64_t dom_hash[6];     // fnv1a of pvac.prf.r.1..3, pvac.prf.noise.1..3 (lpn.hpp:150-157)
    uint64_t toep_hash;       // fnv1a("pvac.dom.toeplitz")
    const uint64_t* s_bits;   // LPN secret (device), s_words u64
    uint32_t s_words, tau_num, tau_den, pad;
};
// one prf_R_core evaluation: an RSeed and a domain index into prf_consts.dom_hash (0..5)
struct prf_request {
    uint64_t ztag, nonce_lo, nonce_hi;
    uint32_t dom;
    uint32_t pad;
};
hipError_t prf_upload_tables(hipStream_t st);
size_t prf_request_bytes();
// n core requests (see k_prf.hip prf_request) -> out[2 n]
hipError_t launch_prf_cores(const prf_consts& k, const void* req, uint64_t n, uint64_t* out, hipStream_t st);
// seeds: 3 u64 per seed {ztag, nonce_lo, nonce_hi}; kind 0..5 one core, 6 prf_R, 7 prf_R_noise.
// req_scratch: 3 n requests; core_scratch: 6 n u64 (kinds 6/7)
hipError_t launch_prf(const prf_consts& k, int kind, const uint64_t* seeds, uint64_t n, void* req_scratch,
                      uint64_t* core_scratch, uint64_t* out, hipStream_t st);
// prf_R of every BASE layer slot of X (slots < n_slots), 0 for others: R_out[2 s], [2 s + 1]
hipError_t launch_base_R(const prf_consts& k, const pvac_ct_batch& X, uint64_t n_slots, void* req_scratch,
                         uint64_t* core_scratch, uint64_t* R_out, hipStream_t st);

// ---- enc_value (k_enc.hip, ops/encrypt.hpp:114-291)
// pre-merge edges per half, 8 signal + 2 Z2 + 3 Z3: two capacity classes of the per-half plan record
// (the default plans and depth hints <= 15 fit the small one; depth hints up to 124 the large one)
constexpr uint32_t kEncPreSmall = 48;
constexpr uint32_t kEncPreMax = 256;
struct enc_plan_args {
    const uint64_t* values;   // n plaintexts
    const uint64_t* rnd;      // csprng_u64 draws: stride words per value
    uint32_t stride;
    uint32_t B, Z2, Z3;
    uint64_t n;
    uint64_t canon;
    const uint64_t* powg;     // B x (lo, hi)
};
size_t enc_half_bytes(uint32_t npre);   // per-half plan record of the capacity class npre needs
// per value: 2 output layers, <= 2 * (8 + 2 Z2 + 3 Z3) edges; cores per value = 2 * 3 * max(Z2 + Z3, 1)
uint32_t enc_cores_per_value(uint32_t Z2, uint32_t Z3);
// 1. draws (exact csprng order), merge groups, shuffle, PRF requests, and the pre-merge edge batch
//    `pre` (2 layers and 2 * npre edge slots per value; salts in pre_salt) for sigma
hipError_t launch_enc_plan(const enc_plan_args& a, void* halves, prf_request* req, pvac_ct_batch& pre,
                           uint64_t* pre_salt, uint32_t* status, hipStream_t st);
// 2. R, noise deltas and the solved coefficients -> pre-merge weights (pre.w_lo / w_hi)
hipError_t launch_enc_weights(const enc_plan_args& a, void* halves, const uint64_t* cores, pvac_ct_batch& pre,
                              hipStream_t st);
// 3. merged groups (fp_add chains, sigma XOR) in shuffled order -> C (2 layers, CSR stride 2 * npre)
hipError_t launch_enc_finish(const enc_plan_args& a, const void* halves, const pvac_ct_batch& pre, pvac_ct_batch& C,
                             uint32_t* status, hipStream_t st);

// ---- enc_items (k_enc_items.hip): a ragged batch of enc_fp_depth / enc_value_depth items, each with
// its own noise plan, plaintext and draw segment. Halves (one enc_fp_depth each) are numbered through
// the batch: item i owns halves [half_off, half_off + halves) = its output layers, and half h owns
// pre-merge edge slots [pre_off + h npre, pre_off + (h + 1) npre): the ragged structure-of-arrays
// scratch (key, salt, r, grp, slot) and the pre-merge batch are both addressed by those slots.
struct enc_item_rec {         // one per item, built and uploaded by the host
    uint64_t v_lo, v_hi;      // plaintext as given (VALUE items: v_lo)
    uint64_t rnd_off;         // the item's draws: rnd[rnd_off .. rnd_off + rnd_cnt)
    uint32_t rnd_cnt;
    uint32_t Z2, Z3;          // its noise plan; npre = 8 + 2 Z2 + 3 Z3 (<= kEncPreMax on the narrow route)
    uint32_t halves;          // 1 = bare enc_fp_depth, 2 = the masked value form
    uint64_t half_off;        // = C.l_off[i]
    uint64_t pre_off;         // = C.e_off[i]
    uint64_t req_off;         // first PRF request; a half takes 3 max(Z2 + Z3, 1)
};
static_assert(sizeof(enc_item_rec) == 64, "enc_item_rec is one cache line");
struct enc_half_hdr {         // one per half, written by k_enc_items_plan
    uint64_t nlo, nhi, ztag;
    uint64_t vlo, vhi;        // the value this half encrypts
    uint64_t pre_off;         // its first pre-edge slot
    uint64_t req_off;         // its first PRF request = its first core
    uint32_t npre, nout;
    uint32_t Z2, Z3;
};
struct enc_items_args {
    uint64_t n;                    // items
    uint64_t n_work;               // entries of `work`
    uint64_t n_halves;
    const enc_item_rec* recs;
    const uint32_t* perm;          // item order of the plan kernel: pre-merge edges (halves x npre) descending
    const uint64_t* work;          // half << 16 | group; group 0 = the signal equation, g + 1 = noise group g
    const uint64_t* rnd;
    const uint64_t* powg;          // B x (lo, hi)
    uint64_t canon;
    uint32_t B, pad;
    enc_half_hdr* hdr;             // [halves]
    uint32_t* key;                 // [pre-edge slots] idx | ch << 16, creation order
    uint64_t* salt;                // ... the make_edge salts (the sigma launch's salts)
    uint64_t *rlo, *rhi;           // ... drawn coefficients (0 where the equations solve them)
    uint8_t *grp, *slot;           // ... compact_edges group of each pre-edge; output slot -> group
};
// 1. per item: draws, merge groups, shuffle, PRF requests, the pre-merge batch `pre` and status
hipError_t launch_enc_items_plan(const enc_items_args& a, prf_request* req, pvac_ct_batch& pre, uint32_t* status,
                                 hipStream_t st);
// 2. per (half, group): R, the group's delta, its solved coefficient, its edges' weights -> pre.w_lo / w_hi
hipError_t launch_enc_items_weights(const enc_items_args& a, const uint64_t* cores, pvac_ct_batch& pre, hipStream_t st);
// 3. per item: merged groups (fp_add chains, sigma XOR) in shuffled order -> C
hipError_t launch_enc_items_finish(const enc_items_args& a, const pvac_ct_batch& pre, pvac_ct_batch& C, uint32_t* status,
                                   hipStream_t st);

// ---- the wide route of enc_items (k_enc_wide.hip, enc_wide.hpp): items whose plan has more than
// kEncPreMax pre-merge edges per half, or every item under PVAC_ENC_WIDE_ALL. A call runs in
// sub-batches of consecutive items; within one, items, halves and pre-edge slots are numbered from the
// sub-batch's first (rec.half_off / pre_off are local), the narrow and the wide items have a record
// list each, and the kernels add base_l / base_e where they write C's offsets. All linear in npre.
struct enc_wide_args {
    uint64_t n;                    // wide items of the sub-batch
    uint64_t n_work, n_fin;
    const enc_item_rec* recs;      // the wide items' records
    const uint32_t* item;          // ... and their item index within the sub-batch
    const uint64_t* work;          // half << 32 | group (as enc_items_args::work, wider)
    const uint64_t* fin;           // half << 32 | first output slot of a chunk of kEncWideFinChunk
    const uint32_t* half_item;     // per half of the sub-batch: item << 1 | h
    const uint64_t* rnd;
    const uint64_t* powg;
    uint64_t canon;
    uint64_t base_l, base_e;       // the sub-batch's first layer and edge slot in C
    uint32_t B;
    uint32_t pre_base;             // the wide items' first entry in the pre-merge batch's index arrays
    enc_half_hdr* hdr;             // [halves of the sub-batch]
    uint32_t* key;                 // [pre-edge slots] as enc_items_args
    uint64_t *salt, *rlo, *rhi;
    uint32_t *occ, *ord;           // ... occurrence number of an edge within its key; edges sorted by key, stable
    uint32_t *gstart, *slot;       // ... per group rank its first entry in ord; output slot -> group rank
    uint32_t* tab;                 // [2 n][2 B] key tables, zeroed before the replay
    uint64_t* dlast;               // [halves][2] the last noise group's Delta
};
// 1. per item, one lane: the draws in order, occurrence numbers and key counts, the shuffle, PRF
//    requests, the pre-merge batch `pre`, C's index entries (at the item's place; C's index arrays and
//    status start at the sub-batch's first item) and status 0 / 1
hipError_t launch_enc_wide_replay(const enc_wide_args& a, prf_request* req, pvac_ct_batch& pre, pvac_ct_batch& C,
                                  uint32_t* status, hipStream_t st);
// 2. per half, one workgroup: ranks and segment starts by a scan of the key table, then the stable sort
hipError_t launch_enc_wide_order(const enc_wide_args& a, hipStream_t st);
// 3. the last group's Delta once per half, then one thread per (half, group) as launch_enc_items_weights
hipError_t launch_enc_wide_weights(const enc_wide_args& a, const uint64_t* cores, pvac_ct_batch& pre, hipStream_t st);
// 4. per output edge, one wave: the fp_add chain over its segment, the sigma XOR, status 2. C's edge and
//    layer arrays start at the sub-batch's first slot.
hipError_t launch_enc_wide_finish(const enc_wide_args& a, const pvac_ct_batch& pre, pvac_ct_batch& C, uint32_t* status,
                                  hipStream_t st);
// the narrow items of a mixed sub-batch: index entries and status from their compact places tmp[t]
// to item nid[t] of C / status, offsets moved by base_l / base_e
hipError_t launch_enc_scatter_index(uint64_t n, const uint32_t* nid, const pvac_ct_batch& tmp, const uint32_t* tmp_status,
                                    uint64_t base_l, uint64_t base_e, pvac_ct_batch& C, uint32_t* status, hipStream_t st);

// ---- dec_value (k_dec.hip):BASE-layer R supplied, PROD R tree, inversions, signed edge sum
size_t dec_scratch_bytes(uint64_t total_layers);
hipError_t launch_dec_value(const pvac_ct_batch& X, const uint64_t* Rbase, const uint64_t* powg, uint32_t Bm,
                            const uint64_t* roff, uint64_t total_layers, void* scratch, uint64_t* out,
                            uint32_t* status, hipStream_t st);

// ---- ct_add / ct_sub over edge_budget (k_add_merge.hip): compact_edges + compact_layers per pair
struct merge_pair_info {
    uint64_t pair, aeo, beo, ceo, nA, nB;
    uint32_t LA, L;
};
size_t merge_scratch_bytes(uint64_t n_edges, uint32_t n_layers);
// counters: 2 device u64 (groups, kept edges) owned by the caller
hipError_t launch_add_merge(const pvac_ct_batch& A, const pvac_ct_batch& B, pvac_ct_batch& C, uint64_t pr,
                            const merge_pair_info& info, uint32_t Bm, int negate_b, void* scratch, size_t scratch_bytes,
                            unsigned long long* counters, hipStream_t st);

// ---- ct_recrypt's parts (k_recrypt.hip): sigma popcounts, ubk_apply, batched compact_edges + compact_layers
// k_compact_small holds one LDS word per cell of a cipher's key space |L| 2B: 56 KiB of cells next to
// 6 KiB of layer and scan tables stays inside the 64 KiB a workgroup gets without opting in. With
// B = 337 that is 21 layers (a recrypt result has 18, a fresh product 8). Ciphers above any of the
// three bounds take launch_add_merge with an empty B.
constexpr uint32_t kCompactSmallCells = 14336;
constexpr uint32_t kCompactSmallLayers = 1024;
constexpr uint32_t kCompactSmallEdges = 1u << 16;
// ones[i] (device, n u64) = popcount over cipher i's e_cnt[i] rows of ceil(m_bits / 64) words
hipError_t launch_sigma_popcount(const pvac_ct_batch& X, uint32_t m_bits, int num_cus, unsigned long long* ones,
                                 hipStream_t st);
// in place on every row of every cipher with active[i] != 0 (active nullable): out bit j = in bit perm[j]
size_t ubk_apply_lds_bytes(uint32_t m_bits);
hipError_t launch_ubk_apply(const pvac_ct_batch& X, const uint32_t* perm, uint32_t m_bits, const uint32_t* active,
                            int num_cus, hipStream_t st);
// compact plan: C.l_off / C.e_off <- X's counts (the caller scans them), cls[i] = PAIR_SMALL / PAIR_LARGE,
// the PAIR_LARGE ids appended to large_ids, stats: n_large, max_keys (cells of the small ones), max_layers
hipError_t launch_compact_plan(const pvac_ct_batch& X, pvac_ct_batch& C, uint32_t Bm, uint8_t* cls, uint64_t* large_ids,
                               plan_stats* stats, hipStream_t st);
// out[8 k] = {id, |L|, |E|, X.e_off, C.e_off, 0, 0, 0} of cipher ids[k]
hipError_t launch_compact_gather(const pvac_ct_batch& X, const pvac_ct_batch& C, const uint64_t* ids, uint64_t n,
                                 uint64_t* out, hipStream_t st);
// every PAIR_SMALL cipher of X -> C (rows, sigma XOR, exact counts); max_cells from the plan
hipError_t launch_compact_small(const pvac_ct_batch& X, pvac_ct_batch& C, const uint8_t* cls, uint32_t Bm, uint32_t m_bits,
                                uint32_t max_cells, hipStream_t st);
// ct_recrypt plumbing: the plan's capacities (C offsets before their scan), verbatim copies of the
// ciphers ids[0, m) and the counts of a view scattered back to C
hipError_t launch_recrypt_plan(const pvac_ct_batch& X, uint64_t max_pl, uint64_t max_pe, pvac_ct_batch& C, hipStream_t st);
hipError_t launch_recrypt_copy(const pvac_ct_batch& X, pvac_ct_batch& C, const uint32_t* ids, uint64_t m, uint32_t m_bits,
                               hipStream_t st);
hipError_t launch_scatter_counts(const uint64_t* l_cnt, const uint64_t* e_cnt, const uint32_t* ids, uint64_t m,
                                 uint64_t* c_l_cnt, uint64_t* c_e_cnt, hipStream_t st);

// ---- commit_ct (k_commit.hip): out[32 i ..] = SHA-256 of cipher i's commit message (commit_msg.hpp).
// head: commit_head_words (14 words); sigma_bytes: bytes of every edge's sigma row that are hashed, 0 =
// weights only; counter: one device u64 the launch zeroes (the lanes draw cipher indices from it)
hipError_t launch_commit_ct(const pvac_ct_batch& X, const uint32_t head[14], uint32_t sigma_bytes, int num_cus,
                            unsigned long long* counter, uint8_t* out, hipStream_t st);

// ---- ct_mul, general path (k_mul_large.hip and the k_large_* files): multi-kernel, global scratch, one workgroup
// per (A-layer, B-layer) product task. The host prepares one descriptor per large pair with
// ABSOLUTE u32-word offsets into one scratch arena (64-bit arrays on even offsets).
constexpr uint32_t kLargeLayersMax = 16384;   // |A.L| + |B.L| + |A.L||B.L| handled in LDS; a pair above is a DEEP pair
static_assert(kLargeLayersMax == PVAC_LAYER_LIMIT_DEFAULT, "the default layer limit is the LDS tables' size");
constexpr uint32_t kLargeDenseMin = 48;       // dense-owner product mode from this many edges

struct large_desc {
    uint64_t pair;               // index of the pair in the batch
    uint64_t n;                  // |A.E| * |B.E|  (< 2^32)
    uint64_t S;                  // |A.L| |B.L| B dense key slots
    uint64_t Lc;                 // |A.L| + |B.L| + |A.L||B.L|  (layers before compaction)
    uint64_t nblk;               // ceil(n / 16) first-insert-time blocks
    uint64_t capE;               // 2 min(n, S) output edge capacity
    fastmod64 nbm;               // libstdc++ bucket count after reserve(n)
    uint32_t LA, LB, nA, nB;
    uint32_t hbits;              // bucket hash table capacity = 2^hbits >= 2 S (dynamic chains only)
    // 1: emit order from per-A-edge counts (o_icnt) instead of the n/16 block marks (o_bmask): static
    // bucket groups, A-layer-major products, 1 <= |B.E| <= 63. The pair falls back to the block marks
    // (cnt[kCntIFail]) when a B layer is too big for the matrix-core mode or an A layer cannot be
    // staged as a dense table
    uint32_t iblk;
    // 1: direct mode (an iblk pair whose scratch holds no per-key sums): k_large_count_la counts the
    // emit positions from key PRESENCE before any multiply, k_large_scan_direct turns the counts into
    // offsets, and k_large_products_direct writes C's edge records at their positions from the
    // matrix-core sums staged in LDS. A pair that turns out to need more (shared buckets, the
    // canonical order, a fallback, a key whose products cancel) is left to the host's redo on the
    // full layout. Its A ids carry the dense cell (k_large_lists)
    uint32_t direct;
    uint32_t pad_d;
    uint64_t nb_m;               // floor(2^32 / |B.E|): t / |B.E| by div_small (k_large.hpp)
    // static bucket groups (bucket_count >= 2 S): per-slot chain head / next of the slots sharing
    // a libstdc++ bucket, word offsets into mul_large_args::grp (kNoGrp: dynamic chains via link)
    uint64_t g_head, g_next;
    // zero-initialised block [o_zero, o_zero + zero_words): cnt | hkey | hhead | bmask | bcnt | used
    uint64_t o_zero, zero_words;
    uint64_t o_cnt;              // [kCntWords] the pair's counters and flags, words kCntNeA .. kCntImg (below)
    uint64_t o_hkey;             // [2^hbits] u64 bucket ids + 1
    uint64_t o_hhead;            // [2^hbits] chain heads (slot + 1)
    uint64_t o_bmask;            // [nblk] u64 per 16 first-insert times: bucket-leader edge codes (2 bits
                                 // per time: 0 none, 1/2 edges, 3 more) | block edges << 32, then the
                                 // block's exclusive suffix offset << 32 (k_large_rank / scan / order)
    uint64_t o_bcnt;             // (unused, empty)
    uint64_t o_used;             // [Lc] product-layer used flags -> compact_layers remap
    // 0xFF-initialised: [S] first-insert time per key slot (INF = key absent)
    uint64_t o_tkey;
    // written before read
    uint64_t o_lstA, o_lstB;     // [2 LA] start,count per layer ++ [nA] edge ids; same for B
    uint64_t o_neA, o_neB;       // [LA] / [LB] non-empty layer lists
    uint64_t o_defer;            // [LA LB] tasks k_large_products_la leaves to k_large_products_defer
                                 // (la << 16 | lb index), counted in cnt[kCntDefer]
    uint64_t o_info;             // [S] ebits (2 bits) | hash slot << 2
    uint64_t o_sums;             // [S] x 4 u64: P lo, P hi, M lo, M hi
    uint64_t o_nxt;              // [S] bucket chain links
    uint64_t o_tb;               // [S] bucket first-insert time
    uint64_t o_within;           // [S] edges of the same bucket emitted before this key
    uint64_t o_etot;             // [S] edges of the bucket (leaders only)
    uint64_t o_cpos;             // [S] canonical positions (guard_budget order)
    uint64_t o_order;            // [capE] emit order: slot << 1 | ch
    uint64_t o_hpos;             // [capE] hash-order index of each canonical-order edge
    uint64_t o_icnt;             // [nA] iblk: edges whose emit time lies in A edge i's product range
                                 // [i |B.E|, (i + 1) |B.E|), then their exclusive suffix offset
    uint64_t o_imask;            // [nA] x 2 u64 iblk: the range's keys with a P edge / an M edge (bit j
                                 // = B edge j), read by k_large_write_ranges; direct pairs: per A layer
                                 // (slice o_lstA's ids offset) the masks of its writer list
    uint64_t o_wle;              // direct pairs: [nA] writer lists, A edge | idx << 21 (k_large_count_la)
    uint64_t o_wln;              // direct pairs: [LA] writer list length per A layer
    // direct pairs: o_icnt holds one count byte per A edge (32-edge groups, 32 B each, zero padded)
    // and o_iwo [ceil(nA / 32)] each group's exclusive suffix offset (k_large_scan_direct)
    uint64_t o_iwo;
    uint64_t words;             // end of this pair's scratch (absolute)
};

struct mul_large_args {
    pvac_ct_batch A, B, C;
    const uint64_t* nonces;
    uint32_t* pair_status;
    const large_desc* desc;      // [nl]
    uint32_t* scratch;           // arena (u32 words)
    uint32_t nl;
    uint32_t Bm;
    uint64_t canon_tag;
    uint64_t edge_budget;
    uint32_t flags;
    uint32_t n_la;               // products: descriptors sel[0, n_la) take k_large_products_la, the rest
                                 // k_large_products (one workgroup per task)
    uint32_t* salt_pos;          // nullable: per output edge slot, its hash-order index
    const uint32_t* grp;         // static bucket-group tables (large_desc::g_head / g_next)
    const uint32_t* sel;         // [nl] descriptor indices, A-layer-major class first
    uint32_t lds_task;           // k_large_products_la: bytes of LDS below its staged B layers (set at launch)
    uint32_t la_per_wg;          // k_large_products_la: A layers per workgroup (max_la_wg = ceil(|A.L| / it))
    uint32_t la_xcd;             // k_large_products_la: 1 = all workgroups of a pair on one XCD (grid y padded to 8)
                                 // (the host always passes 0; the field goes with a measured change to that kernel)
    uint32_t any_dyn;            // some pair has dynamic bucket chains (k_large_link runs)
    uint32_t all_iblk;           // every pair is iblk (rank / order / write on reduced grids)
    uint32_t any_direct;         // some pair is direct (large_desc::direct): the direct kernels run
    uint32_t layers_direct;      // k_large_layers: 1 = the direct pairs' pass (before their products),
                                 // 0 = every other pair (after the products)
    uint32_t all_direct;         // every pair is direct: the per-key kernels are not launched
    uint32_t dir_lb;             // k_large_products_direct: B layers its LDS holds (max |B.L| of the direct pairs)
    uint32_t deep;               // a deep sub-batch: every pair has Lc > kLargeLayersMax (k_large_deep.hip); max_nA is then
                                 // the largest |A.E| or |B.E| of its pairs (the lists kernels' edge grids)
    uint64_t* redo_ids;          // pairs the host re-runs on the full layout (shared with the fresh kernel)
    unsigned int* redo_cnt;
    // chain steps (pvac_hip_ct_mul_chain): a pair whose A_img flag is set holds A as a dense image
    // (k_large_products_direct's image writer) instead of hash-order records; a direct pair of a
    // step with C_img writes C that way when it is dense, and k_large_direct_redo sets its flag
    uint32_t* A_img;             // nullable, [n pairs]
    uint32_t* C_img;             // nullable, [n pairs]
    unsigned long long* img_count;   // nullable: += 1 per pair written as an image
    // launch sizing (maxima over the nl descriptors; max_tasks over the per-task class, max_tasks_all
    // over all, max_la_wg = ceil(|A.L| / kLaPerWG) over the A-layer-major class)
    uint64_t max_S, max_zero, max_tasks, max_capE, max_lay, max_tasks_all, max_la_wg, max_nA;
};
// k_large_products_la: A layers per workgroup; pairs with at most
// kLaMaxLB B layers take it
constexpr uint32_t kLaPerWG = 8;
constexpr uint32_t kLaMaxLB = 4;
hipError_t launch_ct_mul_large(const mul_large_args& a, hipStream_t st);
// a deep sub-batch (mul_large_args::deep) in stages the host can time one by one (k_large_deep.hip):
// 0 init, 1 the lists kernels, 2 products, 3 the layers kernels, 4 link .. write
constexpr int kDeepStages = 5;
hipError_t launch_ct_mul_large_deep(const mul_large_args& a, int stage, hipStream_t st);
// dense chain images back to hash-order records for the listed pairs whose flag is set (the flag is
// cleared): pairs = [n_pairs ids, then n_pairs offsets into tmp], tmp holds 3 words per edge of every
// listed pair (sum of their |A.E|); launches of at most y_cap pairs each (65535: the grid-y limit)
hipError_t launch_image_to_records(const pvac_ct_batch& A, uint32_t* img, const uint64_t* pairs, uint32_t n_pairs,
                                   uint64_t* tmp, uint32_t Bm, uint32_t y_cap, hipStream_t st);
__host__ __device__ inline uint32_t al16(uint32_t x) { return (x + 15u) & ~15u; }
// matrix-core dense mode (k_large_mx.hpp): a task's sparse side is staged as prec | pinf
constexpr int kMxKS = 10;                          // k-steps held in registers: 2 sparse edges each
constexpr uint32_t kMxMaxSparse = 2u * kMxKS;      // sparse sides up to this size take the MFMA path
constexpr uint32_t kMxSparseBytes = 64u * kMxMaxSparse;
constexpr uint32_t kIblkBjtBytes = 4u * 64u;       // k_large_products_la: B edge table of iblk pairs
// LDS of k_large_products_direct for B and nbl staged B layers (the direct mode needs it <= 160 KB;
// the layout is described at the kernel)
__host__ __device__ inline uint32_t dir_lds_base(uint32_t Bm) {   // the digit table, reused by the writer
    // okey [8 B] u16 | obase, oidx, oexc [256] u32 | omk [256] 16 B | part
    return al16(max(32u * Bm, 16u * Bm + 28u * 256u + 64u));
}
__host__ __device__ inline uint32_t dir_lds_bytes(uint32_t Bm, uint32_t nbl) {
    return dir_lds_base(Bm) + nbl * kMxSparseBytes + kIblkBjtBytes + nbl * 32u * Bm;
}
// measured integer-ALU ceilings (k_ubench.hip)
hipError_t run_alu_probe(int kind, int num_cus, hipStream_t st, double* per_s);
hipError_t run_issue_probe(int op, int wps, int num_cus, hipStream_t st, double* per_s, double* clock_hz);
// ct_mul gsum invariant (k_check.hip, utils/metrics.hpp:70-113)
hipError_t launch_check_sizes(const pvac_ct_batch& A, const pvac_ct_batch& B, const pvac_ct_batch& C, unsigned int* mx,
                              hipStream_t st);
hipError_t launch_check_gsum(const pvac_ct_batch& A, const pvac_ct_batch& B, const pvac_ct_batch& C, const uint64_t* nonces,
                             const uint64_t* powg, uint32_t Bm, const unsigned int* mx_host, uint32_t* status,
                             unsigned long long* n_bad, int num_cus, uint8_t* gscratch, hipStream_t st);
// global scratch bytes launch_check_gsum needs when a pair's layer tables exceed LDS (0 if they fit)
uint64_t check_gsum_scratch_bytes(uint32_t Bm, const unsigned int* mx_host, uint64_t n, int num_cus);
// pvac_hip_ct_mul_chain statistics: out[0] += sum |C.E|, out[1] += sum |A.E| |X.E| (k_check.hip)
hipError_t launch_stage_rows(const pvac_ct_batch& src, const pvac_ct_batch& dst, hipStream_t st);
hipError_t launch_chain_stats(const pvac_ct_batch& A, const pvac_ct_batch& X, const pvac_ct_batch& C,
                              unsigned long long* out, hipStream_t st);
constexpr uint64_t kNoGrp = ~0ull;
constexpr uint32_t kCntWords = 16;    // large_desc::o_cnt words
constexpr uint32_t kCntNeA = 0;       // cnt word: non-empty A layers (length of o_neA)
constexpr uint32_t kCntNeB = 1;       // cnt word: non-empty B layers (length of o_neB)
constexpr uint32_t kCntInvalid = 2;   // cnt word: the pair has invalid edges and is rejected (k_large_lists)
constexpr uint32_t kCntTotal = 3;     // cnt word: total output edges (k_large_scan / k_large_scan_direct)
constexpr uint32_t kCntCanonical = 4; // cnt word: the pair takes the canonical (layer, idx, P<M) order
constexpr uint32_t kCntAllocA = 5;    // cnt word: A edge ids allocated to layer lists (k_large_lists)
constexpr uint32_t kCntAllocB = 6;    // cnt word: B edge ids allocated to layer lists
constexpr uint32_t kCntDefer = 7;     // cnt word: tasks in o_defer (k_large_products_la -> _defer)
constexpr uint32_t kCntIFail = 8;    // cnt word: an iblk pair uses the block marks after all
constexpr uint32_t kCntIShared = 9;   // cnt word: an iblk pair has keys sharing a bucket (order probes)
constexpr uint32_t kCntDirect = 10;   // cnt word: a direct pair's positions are final (k_large_scan_direct)
constexpr uint32_t kCntRedo = 11;     // cnt word: a direct pair was handed to the host's redo
constexpr uint32_t kCntImg = 12;      // cnt word: a direct pair writes C as a dense image (k_large_scan_direct)
constexpr uint32_t kCntKept = 13;     // cnt word: a deep pair's kept layers (k_large_layers_deep -> its record writer)
constexpr uint32_t kIblkMaxNB = 63;   // iblk: |B.E| <= 63 (a 64-bit mask per A edge, bit 63 a flag)
// static bucket groups of key slots [0, S) for one bucket count: head[s] = 0 when s is alone in
// its bucket, else the first slot + 1 of the bucket's chain; next[s] = the following slot + 1
// (0 ends). tmp_key / tmp_head: 2^hbits entries, zeroed by the caller.
hipError_t launch_grp_build(fastmod64 nbm, uint32_t Bm, uint64_t S, uint32_t hbits, uint32_t* head, uint32_t* next,
                            unsigned long long* tmp_key, uint32_t* tmp_head, hipStream_t st);

hipError_t launch_ct_add(const pvac_ct_batch& A, const pvac_ct_batch& B, pvac_ct_batch& C, int negate_b,
                         uint32_t max_layers, const uint8_t* pair_class, hipStream_t st);
// the same with the keep / remap table of pair i at slab[C.l_off[i] ..) (k_large_deep.hip): any layer count
hipError_t launch_ct_add_deep(const pvac_ct_batch& A, const pvac_ct_batch& B, pvac_ct_batch& C, int negate_b,
                              uint32_t* slab, const uint8_t* pair_class, hipStream_t st);

// ---- ct_lincomb (k_lincomb.hip): segmented sums of optionally scaled ciphers, the work unit the term.
// Terms of at most kLinWaveLayers layers and kLinWaveEdges edges are closed by a lane group (the
// wave route: a 64-bit keep mask), the others by one workgroup each (a remap table in scratch): the
// workgroup route up to kLinMaxLayers layers, the deep-term route above (deep_ops.hpp has the rule).
constexpr uint64_t kLinKeptMask = (1ull << 40) - 1;   // kraw / sK: kept layers below bit 40, flagged terms above
// segment classes (lincomb_args::cls, pvac_hip_ct_lincomb_status)
enum : uint32_t { LIN_ONE_PASS = 0, LIN_FOLD_BUDGET = 1, LIN_FOLD_CONTRACT = 2 };
struct lincomb_args {
    pvac_ct_batch X, C;
    uint64_t n, n_terms;
    const uint64_t* seg_off;   // [n + 1]
    const uint64_t* term;      // [n_terms]
    const uint64_t* scale;     // nullable, 2 words per term
    const uint32_t* flags;     // nullable
    // context-owned per-term scratch, n_terms + 1 words each (the last one closes the scans)
    uint64_t* sL;              // |X[term].L|, then its exclusive scan: C.l_off[i] = sL[seg_off[i]]
    uint64_t* sE;              // |X[term].E|, then its exclusive scan: term k's edges land at sE[k]
    uint64_t* kraw;            // kept layers | (out of contract ? 1 : 0) << 40
    uint64_t* sK;              // exclusive scan of kraw
    uint64_t* mask;            // wave route: the keep mask
    uint32_t* tseg;            // [n_terms] the term's segment
    uint8_t* troute;           // [n_terms] 0 = wave route, 1 = its remap is in the slab (workgroup and deep-term routes)
    uint64_t* wg_ids;          // [n_terms] the terms beyond the wave route (plan_stats::n_small of them)
    uint32_t* remap;           // the slab: new layer id (0xFFFFFFFF = dropped) at sL[k] + layer
    uint32_t* cls;             // [n] segment class
    uint64_t* fold_ids;        // [n] the fold route's segments (plan_stats::n_large of them)
    // the copy pass's tiles: the term that holds the first layer slot / edge of tile b (kLinLayerTile
    // input layer slots, kLinEdgeTile output edges per workgroup), and n_terms - 1 at the end
    uint32_t* tile_l;
    uint32_t* tile_e;
    plan_stats* stats;
    uint64_t edge_budget;
};
constexpr uint32_t kLinLayerTile = 256;
constexpr uint32_t kLinEdgeTile = 1024;
// plan_stats as the lincomb plan uses it: n_small = workgroup-route terms, n_large = fold segments,
// n_invalid = bad seg_off entries and term indices, max_layers / max_na = largest term |L| / |E|,
// max_prod / max_nb = largest segment layer / edge total, max_buckets = largest fold segment layer
// total (all saturated at 2^32 - 1).
// 1. per term: index check, counts, segment, keep mask of the wave route; seg_off's own checks
hipError_t launch_lincomb_plan(const lincomb_args& a, hipStream_t st);
// 2. (after the scans of sL / sE) the workgroup route's n_wg terms: keep table in LDS -> remap, kraw
hipError_t launch_lincomb_plan_wg(const lincomb_args& a, uint64_t n_wg, uint32_t max_layers, hipStream_t st);
// 2a. a call with a term above kLinMaxLayers: a.wg_ids[0, n_wg) split by lincomb_route into out + 2 (the
//     workgroup route's) and out + 2 + n_terms (the deep-term route's), their counts in out[0] / out[1] (zeroed)
hipError_t launch_lincomb_split(const lincomb_args& a, uint64_t n_wg, uint64_t* out, hipStream_t st);
// 2b. the deep-term route's n_deep terms: keep table and remap in the slab (a.remap), any layer count
hipError_t launch_lincomb_plan_deep(const lincomb_args& a, const uint64_t* deep_ids, uint64_t n_deep, hipStream_t st);
// 3. (after the scan of kraw into sK) per segment: class, fold list, segment maxima
hipError_t launch_lincomb_classify(const lincomb_args& a, hipStream_t st);
// 4. C.l_off / C.e_off and the copy pass's tile tables
hipError_t launch_lincomb_layout(const lincomb_args& a, uint64_t total_layers, uint64_t total_edges, hipStream_t st);
// exec: layers, edges (and sigma rows) of every one-pass segment, then C.l_cnt / C.e_cnt
hipError_t launch_lincomb_copy(const lincomb_args& a, uint64_t total_layers, uint64_t total_edges, hipStream_t st);

// ---- metrics (k_metrics.hip, utils/metrics.hpp:43-86)
// hist[256 i + b] (device u64) = bytes equal to b among the first ceil(m_bits / 64) words of cipher i's
// sigma rows; every entry is written. *wide_out: 1 = the 16-byte-load path served the call, 0 = the 8-byte one
hipError_t launch_sigma_bytehist(const pvac_ct_batch& X, uint32_t m_bits, int num_cus, unsigned long long* hist, int* wide_out,
                                 hipStream_t st);
// layer_gsum's size pass: out (8 device u64, zeroed by the caller) = most layers of a cipher whose table
// lives in dynamic LDS, most layers of a cipher that needs a global slab, ciphers on the wave / workgroup /
// large route, ciphers that need a slab, ciphers beyond 2^28 layers (refused by the host)
constexpr int kGsumSizeWords = 8;
hipError_t launch_gsum_sizes(const pvac_ct_batch& X, unsigned long long* out, hipStream_t st);
// global scratch the launch needs for these sizes (0: every table fits LDS)
uint64_t gsum_slab_bytes(uint64_t n, const unsigned long long* sizes_host, int num_cus);
// gsum[2 (l_off[i] + l)], [.. + 1] = agg_layer_gsum(X_i, l) for l < l_cnt[i]; status nullable;
// ticket: one device u64 (the slab counter, zeroed by the launch)
hipError_t launch_layer_gsum(const pvac_ct_batch& X, const uint64_t* powg, uint32_t Bm, const unsigned long long* sizes_host,
                             uint64_t* gsum, uint32_t* status, uint8_t* slabs, unsigned long long* ticket, int num_cus,
                             hipStream_t st);

// ---- device .ct codec (k_ct_image.hip, ct_image.hpp): a resident batch <-> a .ct file image in device memory
// ctl: device words the passes report in and the parse's row kernels read their go-ahead from.
//   plan : 0 = sum of the cipher sizes (image bytes - 16), 1 = edge tiles, 2 = layers with a rule >= 256,
//          3 = edges of the largest tile
//   parse: 0 / 1 = layer and edge totals, 2 = edge tiles, 3 = malformed ciphers, 4 = edges whose nbits differs
constexpr int kCtImageCtlWords = 8;
// sizes of X's image: pos (n + 1), and toff (n; the exclusive scan of the per-cipher edge tile counts);
// sz: n words of scratch. Nothing is read back here.
hipError_t launch_ct_image_plan(const pvac_ct_batch& X, uint32_t nbits, uint64_t* sz, uint64_t* toff, uint64_t* scan_scratch,
                                unsigned long long* ctl, uint64_t* pos, hipStream_t st);
// image[0, pos[n]) from X with the plan's pos / toff / tile count / largest tile; wide: sigma rows by 16-byte loads
hipError_t launch_ct_image_write(const pvac_ct_batch& X, uint32_t nbits, const uint64_t* pos, const uint64_t* toff,
                                 uint64_t ntiles, uint32_t max_tile_edges, bool wide, int num_cus, uint8_t* image, hipStream_t st);
// validation, scans and the row kernels (which write X only when ctl says every cipher is well-formed
// and the totals fit the caps); words: 5 (n + 1) words of scratch; wide: sigma rows by 16-byte stores
hipError_t launch_ct_image_parse(const uint8_t* image, uint64_t len, const uint64_t* pos, uint64_t n, uint32_t nbits,
                                 const pvac_ct_batch& X, uint64_t layer_cap, uint64_t edge_cap, uint32_t* status, uint64_t* words,
                                 uint64_t* scan_scratch, unsigned long long* ctl, bool wide, int num_cus, hipStream_t st);

// ---- batch_gather (k_gather.hip, gather_tiles.hpp): whole ciphers of several resident batches into one dense batch
// ctl: 0 / 1 = layer and edge totals, 2 = tiles of a weights-only copy, 3 = picks out of range, 4 = tiles with sigma
constexpr int kGatherCtlWords = 5;
// The plan's own arrays, m entries each: the picked ciphers' counts (cL, cE), their dense offsets in the
// output (oL, oE: the scans of the counts), the scans of the tile counts of a weights-only copy (toff,
// geometry g) and of a copy with sigma rows (toff_s, geometry gs; null when the sources cannot give sigma:
// dst's rows, sigma included, are allocated between plan and exec, so the plan deals for both), the
// source's row offsets (sL, sE) and the source index (src).
struct gather_plan_args {
    const pvac_ct_batch* srcs;   // DEVICE table of the n_src source descriptors
    const uint64_t* first;       // DEVICE, n_src + 1: first output of source j in a concatenation
    uint32_t n_src;
    gather_geom g, gs;
    uint64_t m;
    const uint32_t* pick_src;    // nullable
    const uint64_t* pick_idx;    // null: concatenation
    uint64_t *cL, *cE, *oL, *oE, *toff, *toff_s, *sL, *sE;
    uint32_t* src;
    unsigned long long* ctl;
};
struct gather_exec_args {
    const pvac_ct_batch* srcs;
    pvac_ct_batch dst;           // row arrays (sigma null: no sigma rows are copied)
    const uint64_t *cL, *cE, *oL, *oE, *toff, *sL, *sE;   // toff: the table of g's geometry
    const uint32_t* src;
    uint64_t m, ntiles;
    gather_geom g;
};
// the pick pass, the scans and, when every pick is in range, dst's four index arrays; nothing is read back here
hipError_t launch_gather_plan(const gather_plan_args& a, const pvac_ct_batch& dst, uint64_t* scan_scratch, hipStream_t st);
// the rows of every tile; wide: sigma rows by 16-byte pieces (gather_sigma_wide)
hipError_t launch_gather_rows(const gather_exec_args& a, bool wide, int num_cus, hipStream_t st);

}  // namespace pvhip
