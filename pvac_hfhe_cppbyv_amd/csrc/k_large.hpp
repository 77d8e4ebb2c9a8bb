// k_large.hpp — device-side pieces of the general ct_mul path that at least two of its kernel files
// use (k_mul_large.hip, k_large_products.hip, k_large_direct.hip, k_large_aux.hip, k_large_deep.hip);
// included only by them. The host-visible interface is in common.hpp.
#pragma once
#include "common.hpp"
#include "sha256.hpp"

#ifdef PVAC_DIR_STAMPS   // diagnostic build only: the direct kernels' wave 0 s_memtime per phase (k_large_direct.hip)
__device__ __forceinline__ unsigned long long dir_stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define DSTAMP(ph) do { const unsigned long long t_ = dir_stamp(); st_acc[ph] += t_ - t_prev; t_prev = t_; } while (0)
#else
#define DSTAMP(ph) do {} while (0)
#endif

namespace pvhip {

namespace {

constexpr uint32_t kInf = 0xFFFFFFFFu;
constexpr uint32_t kIblkMaxSparse = 20;   // == kMxMaxSparse: B layers the matrix-core mode takes
constexpr int kLB = 256;            // threads per workgroup (task / grid-stride kernels)
constexpr int kLBig = 1024;         // threads per workgroup (per-pair kernels)

__device__ __forceinline__ uint64_t* w64(uint32_t* s, uint64_t o) { return (uint64_t*)(s + o); }

__device__ __forceinline__ uint32_t mod_small(uint32_t x, uint32_t B) { return x >= B ? x - B : x; }

// a bucket leader with first-insert time t and E > 0 edges: its 2-bit edge code lands in the u64
// of its 16-time block (times are unique, so the add is an OR) and E in the block's count
__device__ __forceinline__ void leader_mark(unsigned long long* bpack, uint32_t t, uint32_t E) {
    const uint64_t code = E < 3u ? E : 3u;
    atomicAdd(&bpack[t >> 4], ((unsigned long long)E << 32) | (code << (2u * (t & 15u))));
}

// static bucket groups (large_desc::g_head): 0 = the key is alone in its libstdc++ bucket
__device__ __forceinline__ const uint32_t* group_heads(const mul_large_args& g, const large_desc& d) {
    return d.g_head != kNoGrp ? g.grp + d.g_head : nullptr;
}

// iblk pairs leave tkey unset in the layer pairs (la, lb) with no edges on one side: no products
// there, so no keys; the passes that walk every slot skip them
__device__ __forceinline__ bool iblk_dead(const uint32_t* S, const large_desc& d, uint64_t s, uint32_t Bm) {
    if (!d.iblk) return false;
    const uint32_t lp = (uint32_t)s / Bm, la = lp / d.LB, lb = lp - la * d.LB;
    return S[d.o_lstA + d.LA + la] == 0u || S[d.o_lstB + d.LB + lb] == 0u;
}

// one edge of a layer: its words and its index in the pair's edge array (first-insert times use it)
struct edge_rec {
    uint64_t meta, lo, hi;
    uint32_t e;
};
// the edges of one layer of one side of a pair, gathered through the layer's id list (layer-grouped
// 32-byte records written by k_large_lists were measured: the scattered record writes cost lists
// more than the products kernel saved)
struct layer_src {
    const pvac_ct_batch* X;
    uint64_t eo;          // the pair's edge offset in X
    const uint32_t* ids;
    uint32_t n;
};
__device__ __forceinline__ edge_rec load_edge(const layer_src& L, uint32_t k) {
    const uint32_t e = L.ids[k];
    return edge_rec{L.X->meta[L.eo + e], L.X->w_lo[L.eo + e], L.X->w_hi[L.eo + e], e};
}
__device__ __forceinline__ layer_src side_layer(const pvac_ct_batch* X, uint64_t eo, const uint32_t* S, uint64_t o_lst, uint32_t L,
                                                uint32_t l) {
    return layer_src{X, eo, S + o_lst + 2u * L + S[o_lst + l], S[o_lst + L + l]};
}

// ---------------------------------------------------------------- layers
// A pair's uncompacted layer list A || B || products (|A.L| + |B.L| + |A.L||B.L| entries): B's PROD
// parents shifted by |A.L|, product layer lp = la |B.L| + lb a PROD of la and |A.L| + lb. Both are for
// the files that run compact_layers over the list (k_mul_large.hip, k_large_deep.hip).
__device__ __forceinline__ void layer_parents(const mul_large_args& g, uint64_t alo, uint64_t blo, uint32_t LA,
                                              uint32_t LB, uint32_t l, uint32_t& rule, uint32_t& pa, uint32_t& pb) {
    const uint32_t base = LA + LB;
    if (l < LA) {
        const pvac_layer& x = g.A.layers[alo + l];
        rule = x.rule; pa = x.pa; pb = x.pb;
    } else if (l < base) {
        const pvac_layer& x = g.B.layers[blo + (l - LA)];
        rule = x.rule; pa = x.pa + LA; pb = x.pb + LA;
    } else {
        rule = 1; pa = (l - base) / LB; pb = LA + (l - base) % LB;
    }
}

// layer l's record before the remap; a product layer's nonce is the one drawn for its slot of C, its
// ztag is computed here (so only for the layers a caller keeps)
__device__ __forceinline__ pvac_layer layer_record(const mul_large_args& g, uint64_t alo, uint64_t blo, uint64_t clo,
                                                   uint32_t LA, uint32_t LB, uint32_t l) {
    const uint32_t base = LA + LB;
    pvac_layer y;
    if (l < LA) {
        y = g.A.layers[alo + l];
    } else if (l < base) {
        y = g.B.layers[blo + (l - LA)];
        if (y.rule == 1) { y.pa += LA; y.pb += LA; }
    } else {
        const uint32_t lp = l - base;
        const uint64_t slot = clo + l;
        y.rule = 1; y.pad = 0;
        y.pa = lp / LB; y.pb = LA + lp % LB;
        y.nonce_lo = g.nonces[2 * slot];
        y.nonce_hi = g.nonces[2 * slot + 1];
        y.ztag = layer_ztag(g.canon_tag, y.nonce_lo, y.nonce_hi);
    }
    return y;
}

// ---------------------------------------------------------------- products
constexpr int kLP = 384;                // products workgroup: one lane per output index r (B = 337)
constexpr int kLPX = 256;                // products workgroup with the matrix-core dense mode (4 waves)
constexpr int kLaMinBlocks = 4;          // resident workgroups per CU the A-layer-major kernels are compiled for
constexpr int kLPRows = 3;               // B <= kLP * kLPRows
constexpr uint32_t kBmax = kLP * kLPRows;
#ifdef PVAC_ASM_MARKS   // ISA census builds only (tools/asm_phases.py)
#define MXMARK(ph) asm volatile("; PVAC_MARK " #ph ::: "memory")
#else
#define MXMARK(ph) do {} while (0)
#endif

// a loaded value kept in a VGPR until here: a uniform load is otherwise moved to an SGPR right
// after it is issued, and that readfirstlane waits for every load in flight
__device__ __forceinline__ uint32_t late(uint32_t x) {
    asm volatile("" : "+v"(x));
    return x;
}

// t = i D + j for D <= 63: m = floor(2^32 / D), i = (t m) >> 32 is i or i - 1
__device__ __forceinline__ uint32_t div_small(uint32_t t, uint32_t D, uint64_t m, uint32_t& j) {
    uint32_t i = (uint32_t)(((uint64_t)t * m) >> 32);
    uint32_t r = t - i * D;
    if (r >= D) {
        ++i;
        r -= D;
    }
    j = r;
    return i;
}

inline unsigned grid_x(uint64_t work, uint64_t per_block, uint64_t cap) {
    uint64_t b = (work + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

}  // namespace

// the products stages of launch_ct_mul_large (k_mul_large.hip), each in its kernels' file
// direct pairs (k_large_direct.hip): k_large_count_la and k_large_scan_direct (sets b.lds_task), then,
// after the direct pairs' k_large_layers pass, k_large_products_direct and k_large_direct_redo
void launch_large_direct_count(mul_large_args& b, hipStream_t st);
void launch_large_direct_products(const mul_large_args& b, hipStream_t st);
// every other pair (k_large_products.hip): k_large_products, k_large_products_la, k_large_products_defer
void launch_large_products(const mul_large_args& a, hipStream_t st);
// k_mul_large.hip's stages around the deep kernels (k_large_deep.hip): k_large_init; link, rank, scan,
// order and write with dynamic bucket chains
void launch_large_init(const mul_large_args& a, hipStream_t st);
void launch_large_emit(const mul_large_args& a, hipStream_t st);

}  // namespace pvhip
