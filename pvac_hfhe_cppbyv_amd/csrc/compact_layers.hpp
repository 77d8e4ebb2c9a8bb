// compact_layers.hpp — the reference's compact_layers (ops/encrypt.hpp:73-104), stated once for the
// device: mark the layers used by edges, close the marks over PROD parents, turn the flags into a
// remap by an exclusive count, rewrite the kept layer records and the edges' layer ids. Device-only;
// included by the kernel files whose kernels run the routine (the fresh ct_mul kernel keeps its own).
//
// Wave form: a cipher of at most 64 layers, one group of G lanes, the keep set a 64-bit mask.
// Workgroup form: a table of one word per layer, in LDS or in global memory, one workgroup per cipher.
//
// Barrier and visibility contract of the workgroup form:
//   - A sweep's stores are plain stores of 1 and race harmlessly: a lane that misses a mark made in
//     the same sweep leaves its layer to the next sweep, which runs because the marking lane set
//     `changed`; a lane that repeats a mark stores the same 1.
//   - `changed` is cleared by thread 0 between two barriers and read by every thread after one.
//   - Table words that one thread stored and another thread reads have a barrier between the two:
//     block_close begins with one (the caller's marks need none of their own), block_remap ends with
//     one (the remap is readable when it returns). That holds for a table in global memory too: a
//     workgroup runs on one CU, and a barrier orders its global stores before its later loads.
//   - Plain pointers everywhere, no `volatile`: every loop that reads the table stands between two
//     barriers, which the compiler moves no memory access across, and inside a sweep a value held in
//     a register is just the missed mark of the first point. The host-checked layer counts bound every
//     index; a parent id beyond the table is never followed.
#pragma once
#include "common.hpp"

namespace pvhip {

namespace {

constexpr uint32_t kDropped = 0xFFFFFFFFu;   // remap entry, layer id or parent id of a dropped layer

// ---------------------------------------------------------------- wave form
template <int G>
__device__ __forceinline__ uint64_t group_or_u64(uint64_t v) {
#pragma unroll
    for (int d = 1; d < G; d <<= 1) v |= (uint64_t)__shfl_xor((long long)v, d, 64);
    return v;
}

// The keep mask of a group's cipher: `used` (uniform over the group) closed over PROD parents
// (encrypt.hpp:80-93). Lane l of the group passes layer l's parents as a mask (0: no PROD layer).
// Depth-bounded by the layer count; the wave stops when every group has reached its fixed point, so
// all groups of a wave, dead ones included, reach the same shuffles.
template <int G>
__device__ __forceinline__ uint64_t group_close(uint64_t used, uint64_t my_parent_mask, uint32_t l) {
    uint64_t keep = used;
    for (;;) {
        const uint64_t nk = keep | group_or_u64<G>(((keep >> l) & 1ull) ? my_parent_mask : 0ull);
        const bool moved = nk != keep;
        keep = nk;
        if (!__any(moved)) break;
    }
    return keep;
}

// ---------------------------------------------------------------- workgroup form
// keep[0, L): nonzero = used. Parallel sweeps until stable (any parent order). parents(l, rule, pa,
// pb) gives layer l's rule and parent ids in the table's numbering; it is called for kept layers only.
template <int BS, class Parents>
__device__ __forceinline__ void block_close(uint32_t* keep, uint32_t L, uint32_t* changed, Parents parents) {
    const uint32_t tid = threadIdx.x;
    for (;;) {
        __syncthreads();
        if (tid == 0) *changed = 0;
        __syncthreads();
        for (uint32_t l = tid; l < L; l += BS) {
            if (!keep[l]) continue;
            uint32_t rule, pa, pb;
            parents(l, rule, pa, pb);
            if (rule != 1) continue;
            if (pa < L && !keep[pa]) { keep[pa] = 1; *changed = 1; }
            if (pb < L && !keep[pb]) { keep[pb] = 1; *changed = 1; }
        }
        __syncthreads();
        if (!*changed) break;
    }
}

// flags[0, L) (0 / 1) -> dst[0, L): the exclusive count of kept layers, kDropped for the others;
// returns the kept count. dst may be flags. Tiles of kRemapPer * BS layers in index order, thread t
// on layers kRemapPer * t .. of the tile: consecutive lanes on consecutive words, for a table in
// global memory as in LDS. `part` is LDS scratch of BS / 64 words.
constexpr uint32_t kRemapPer = 4;
template <int BS>
__device__ __forceinline__ uint32_t block_remap(const uint32_t* flags, uint32_t* dst, uint32_t L, uint32_t* part) {
    uint32_t kept = 0;
    for (uint32_t b0 = 0; b0 < L; b0 += kRemapPer * BS) {
        const uint32_t l0 = b0 + kRemapPer * threadIdx.x;
        uint32_t v[kRemapPer];
        uint32_t local = 0;
#pragma unroll
        for (uint32_t k = 0; k < kRemapPer; ++k) {
            v[k] = l0 + k < L ? flags[l0 + k] : 0u;
            local += v[k];
        }
        uint32_t tot;
        uint32_t run = kept + block_exclusive_scan<BS>(local, part, tot);
#pragma unroll
        for (uint32_t k = 0; k < kRemapPer; ++k) {
            if (l0 + k < L) dst[l0 + k] = v[k] ? run : kDropped;
            run += v[k];
        }
        kept += tot;
    }
    __syncthreads();
    return kept;
}

// ---------------------------------------------------------------- A || B (ct_add, ct_sub, the merge path)
// the layers of a pair's two ciphers as one list: A's, then B's with their PROD parents shifted by |A.L|
struct ab_layers {
    const pvac_layer *a, *b;   // the pair's records
    uint32_t LA;
    __device__ __forceinline__ pvac_layer at(uint32_t l) const {
        if (l < LA) return a[l];
        pvac_layer y = b[l - LA];
        if (y.rule == 1) { y.pa += LA; y.pb += LA; }
        return y;
    }
    __device__ __forceinline__ void operator()(uint32_t l, uint32_t& rule, uint32_t& pa, uint32_t& pb) const {
        const pvac_layer& x = l < LA ? a[l] : b[l - LA];
        const uint32_t off = l < LA ? 0u : LA;
        rule = x.rule; pa = x.pa + off; pb = x.pb + off;
    }
};
__device__ __forceinline__ ab_layers pair_layers(const pvac_ct_batch& A, const pvac_ct_batch& B, uint64_t pr) {
    return ab_layers{A.layers + A.l_off[pr], B.layers + B.l_off[pr], (uint32_t)A.l_cnt[pr]};
}

// a kept record's parents through the remap (left alone when the remap is the identity)
__device__ __forceinline__ void remap_parents(pvac_layer& y, const uint32_t* remap, uint32_t L, bool identity) {
    if (identity || y.rule != 1) return;
    y.pa = y.pa < L ? remap[y.pa] : kDropped;
    y.pb = y.pb < L ? remap[y.pb] : kDropped;
}

// the kept records of an A || B list to out[remap[l]], by the whole workgroup
template <int BS>
__device__ __forceinline__ void write_ab_layers(const ab_layers& s, pvac_layer* out, const uint32_t* remap, uint32_t L,
                                                bool identity) {
    for (uint32_t l = threadIdx.x; l < L; l += BS) {
        const uint32_t to = remap[l];
        if (to == kDropped) continue;
        pvac_layer y = s.at(l);
        remap_parents(y, remap, L, identity);
        out[to] = y;
    }
}

// ---------------------------------------------------------------- sigma rows
// ct_add's sigma carry: A's rows then B's to C's, 16 bytes per work item, `stride` work items of
// which this is number `first`
__device__ __forceinline__ void carry_sigma_rows(const pvac_ct_batch& A, const pvac_ct_batch& B, const pvac_ct_batch& C,
                                                 uint64_t aeo, uint64_t beo, uint64_t ceo, uint64_t nA, uint64_t nB,
                                                 uint32_t first, uint32_t stride) {
    if (!(C.sigma && A.sigma && B.sigma)) return;
    const uint32_t sw = C.sigma_words;
    const uint64_t chunks_per_edge = sw / 2;
    const uint64_t total = (nA + nB) * chunks_per_edge;
    for (uint64_t c = first; c < total; c += stride) {
        const uint64_t e = c / chunks_per_edge, k = c - e * chunks_per_edge;
        const bool fromB = e >= nA;
        const ulonglong2* srcp = fromB ? (const ulonglong2*)(B.sigma + (beo + (e - nA)) * B.sigma_words)
                                       : (const ulonglong2*)(A.sigma + (aeo + e) * A.sigma_words);
        ((ulonglong2*)(C.sigma + (ceo + e) * sw))[k] = srcp[k];
    }
}

}  // namespace

}  // namespace pvhip
