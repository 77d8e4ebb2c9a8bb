// k_large_deep.hip — the general ct_mul path and ct_add / ct_sub for DEEP ciphers: pairs whose layer
// count is beyond the LDS tables of k_large_lists / k_large_layers (Lc = |A.L| + |B.L| + |A.L||B.L| >
// kLargeLayersMax) or of k_ct_add (|A.L| + |B.L| > 30000). Nothing here sizes an LDS array by a layer
// count: the per-layer tables live in the pair's global scratch, layer ids are full 32-bit words.
//
// ct_mul: a deep pair runs the dynamic route of k_mul_large.hip (bucket table + chains, per-key sums)
// with its lists and layers stages replaced:
//   lists  : the histogram and the cursors of the per-layer edge lists live in used[0, |A.L| + |B.L|):
//            k_large_init zeroed it, and nothing reads it before the layers stage, which starts from
//            used[l >= |A.L| + |B.L|] alone. Three grid-stride kernels over the pair's edges, layers
//            and edges again (hist, alloc, scatter); the scatter pass reads the metas again (no packed
//            copy of a layer id). The lists' contents are what k_large_lists leaves for a pair that is
//            neither an image nor direct: lstA / lstB (start, count), neA / neB, idsA / idsB, four
//            counters; orders inside a list are arrival orders there too.
//   layers : one workgroup per pair closes the keep flags in place in used[] (any parent order: sweeps
//            to a fixed point, encrypt.hpp:80-88), scans them into the remap in place (tiles in index
//            order: deterministic), and a grid-stride kernel writes the kept records.
// ct_add: k_ct_add with its keep / remap table at slab[C.l_off[pair] ..): C.l_off is the exclusive scan
// of |A.L| + |B.L|, so one slab of the plan's total_layer_slots words serves the batch.
#include "k_large.hpp"
#include "sha256.hpp"

namespace pvhip {

namespace {

// ---------------------------------------------------------------- lists
// edges -> per-layer counts in used[0, LA + LB); an edge with layer >= |L|, idx >= B or ch > 1 marks
// the pair invalid (every writer stores 1)
__global__ __launch_bounds__(kLB) void k_large_lists_deep_hist(mul_large_args g) {
    const large_desc& d = g.desc[blockIdx.y];
    const uint64_t pr = d.pair;
    const uint32_t LA = d.LA, LB = d.LB, nA = d.nA, nB = d.nB, Bm = g.Bm;
    const uint64_t aeo = g.A.e_off[pr], beo = g.B.e_off[pr];
    uint32_t* S = g.scratch;
    uint32_t* hist = S + d.o_used;
    const uint64_t stride = (uint64_t)gridDim.x * kLB;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kLB + threadIdx.x; i < nA; i += stride) {
        const uint64_t m = g.A.meta[aeo + i];
        const uint32_t la = meta_layer(m);
        if (la >= LA || meta_idx(m) >= Bm || meta_ch(m) > 1) bad = true;
        else atomicAdd(&hist[la], 1u);
    }
    for (uint64_t j = (uint64_t)blockIdx.x * kLB + threadIdx.x; j < nB; j += stride) {
        const uint64_t m = g.B.meta[beo + j];
        const uint32_t lb = meta_layer(m);
        if (lb >= LB || meta_idx(m) >= Bm || meta_ch(m) > 1) bad = true;
        else atomicAdd(&hist[LA + lb], 1u);
    }
    if (bad) S[d.o_cnt + kCntInvalid] = 1;
}

// layers -> list ranges by atomic allocation, non-empty layer lists by atomic append, cursors in
// place of the counts; an invalid pair is rejected here (reference behaviour is UB)
__global__ __launch_bounds__(kLB) void k_large_lists_deep_alloc(mul_large_args g) {
    const large_desc& d = g.desc[blockIdx.y];
    const uint64_t pr = d.pair;
    const uint32_t LA = d.LA, LB = d.LB;
    uint32_t* S = g.scratch;
    uint32_t* cnt = S + d.o_cnt;
    if (cnt[kCntInvalid]) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            g.pair_status[pr] = 2;
            g.C.l_cnt[pr] = 0;
            g.C.e_cnt[pr] = 0;
        }
        return;
    }
    uint32_t* hist = S + d.o_used;
    const uint64_t stride = (uint64_t)gridDim.x * kLB;
    for (uint64_t l = (uint64_t)blockIdx.x * kLB + threadIdx.x; l < (uint64_t)LA + LB; l += stride) {
        const uint32_t c = hist[l];
        const bool a = l < LA;
        uint32_t* lst = a ? S + d.o_lstA : S + d.o_lstB;
        const uint32_t ll = a ? (uint32_t)l : (uint32_t)l - LA;
        const uint32_t L = a ? LA : LB;
        uint32_t start = 0;
        if (c) {
            start = atomicAdd(&cnt[a ? kCntAllocA : kCntAllocB], c);
            const uint32_t k = atomicAdd(&cnt[a ? kCntNeA : kCntNeB], 1u);
            (S + (a ? d.o_neA : d.o_neB))[k] = ll;
        }
        lst[ll] = start;
        lst[L + ll] = c;
        hist[l] = start;   // cursor
    }
}

// edges -> their layer's id list (the metas read again: full 32-bit layer ids)
__global__ __launch_bounds__(kLB) void k_large_lists_deep_scatter(mul_large_args g) {
    const large_desc& d = g.desc[blockIdx.y];
    const uint64_t pr = d.pair;
    const uint32_t LA = d.LA, LB = d.LB, nA = d.nA, nB = d.nB;
    uint32_t* S = g.scratch;
    if (S[d.o_cnt + kCntInvalid]) return;
    const uint64_t aeo = g.A.e_off[pr], beo = g.B.e_off[pr];
    uint32_t* cur = S + d.o_used;
    uint32_t* idsA = S + d.o_lstA + 2 * (uint64_t)LA;
    uint32_t* idsB = S + d.o_lstB + 2 * (uint64_t)LB;
    const uint64_t stride = (uint64_t)gridDim.x * kLB;
    for (uint64_t i = (uint64_t)blockIdx.x * kLB + threadIdx.x; i < nA; i += stride)
        idsA[atomicAdd(&cur[meta_layer(g.A.meta[aeo + i])], 1u)] = (uint32_t)i;
    for (uint64_t j = (uint64_t)blockIdx.x * kLB + threadIdx.x; j < nB; j += stride)
        idsB[atomicAdd(&cur[LA + meta_layer(g.B.meta[beo + j])], 1u)] = (uint32_t)j;
}

// ---------------------------------------------------------------- compact_layers
// rule and parents of layer l of the pair's uncompacted layer list (A's, B's shifted, the products)
__device__ __forceinline__ void deep_parents(const mul_large_args& g, uint64_t alo, uint64_t blo, uint32_t LA, uint32_t LB,
                                             uint32_t l, uint32_t& rule, uint32_t& pa, uint32_t& pb) {
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

// One workgroup per pair (encrypt.hpp:73-104), in place in used[0, Lc): keep flags = product layers
// with emitted edges (the products stage's marks), closed over PROD parents; then flag -> remap
// (exclusive count of kept layers, kInf = dropped). The workgroup's own global stores are read back
// after barriers only.
__global__ __launch_bounds__(kLBig) void k_large_layers_deep(mul_large_args g) {
    __shared__ uint32_t changed;
    __shared__ uint32_t part[kLBig / 64];
    const large_desc& d = g.desc[blockIdx.x];
    uint32_t* S = g.scratch;
    if (S[d.o_cnt + kCntInvalid]) return;
    const uint64_t pr = d.pair;
    const uint32_t LA = d.LA, LB = d.LB, Lc = (uint32_t)d.Lc, base = LA + LB;
    const uint64_t alo = g.A.l_off[pr], blo = g.B.l_off[pr];
    uint32_t* used = S + d.o_used;
    const uint32_t tid = threadIdx.x;
    for (uint32_t l = tid; l < Lc; l += kLBig) used[l] = l >= base ? (used[l] != 0 ? 1u : 0u) : 0u;
    for (;;) {
        __syncthreads();
        if (tid == 0) changed = 0;
        __syncthreads();
        for (uint32_t l = tid; l < Lc; l += kLBig) {
            if (!used[l]) continue;
            uint32_t rule, pa, pb;
            deep_parents(g, alo, blo, LA, LB, l, rule, pa, pb);
            if (rule != 1) continue;
            if (pa < Lc && !used[pa]) { used[pa] = 1; changed = 1; }
            if (pb < Lc && !used[pb]) { used[pb] = 1; changed = 1; }
        }
        __syncthreads();
        if (!changed) break;
    }
    // tiles of 4 kLBig layers in index order: thread t takes layers 4t .. 4t + 3 of the tile
    uint32_t total = 0;
    for (uint32_t b0 = 0; b0 < Lc; b0 += 4u * kLBig) {
        const uint32_t l0 = b0 + 4u * tid;
        uint32_t v[4];
        uint32_t local = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            v[k] = l0 + k < Lc ? used[l0 + k] : 0u;
            local += v[k];
        }
        uint32_t tot;
        uint32_t run = total + block_exclusive_scan<kLBig>(local, part, tot);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (l0 + k < Lc) used[l0 + k] = v[k] ? run : kInf;
            run += v[k];
        }
        total += tot;
    }
    if (tid == 0) {
        S[d.o_cnt + kCntKept] = total;
        g.C.l_cnt[pr] = total;
    }
}

// the kept layer records from the remap (product-layer ztags for kept layers only; parents remapped
// unless the remap is the identity)
__global__ __launch_bounds__(kLB) void k_large_layers_deep_write(mul_large_args g) {
    const large_desc& d = g.desc[blockIdx.y];
    uint32_t* S = g.scratch;
    if (S[d.o_cnt + kCntInvalid]) return;
    const uint64_t pr = d.pair;
    const uint32_t LA = d.LA, LB = d.LB, Lc = (uint32_t)d.Lc, base = LA + LB;
    const uint64_t alo = g.A.l_off[pr], blo = g.B.l_off[pr], clo = g.C.l_off[pr];
    const uint32_t* remap = S + d.o_used;
    const bool identity = S[d.o_cnt + kCntKept] == Lc;
    const uint64_t stride = (uint64_t)gridDim.x * kLB;
    for (uint64_t lw = (uint64_t)blockIdx.x * kLB + threadIdx.x; lw < Lc; lw += stride) {
        const uint32_t l = (uint32_t)lw;
        const uint32_t to = remap[l];
        if (to == kInf) continue;
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
        if (!identity && y.rule == 1) {
            y.pa = y.pa < Lc ? remap[y.pa] : kInf;
            y.pb = y.pb < Lc ? remap[y.pb] : kInf;
        }
        g.C.layers[clo + to] = y;
    }
}

// ---------------------------------------------------------------- ct_add / ct_sub
constexpr int kAddDeepBlock = 1024;

// k_ct_add (k_ct.hip) with the keep flags, then the remap, in the pair's slab words
__global__ __launch_bounds__(kAddDeepBlock) void k_ct_add_deep(pvac_ct_batch A, pvac_ct_batch B, pvac_ct_batch C, int negate_b,
                                                              uint32_t* slab, const uint8_t* pair_class) {
    __shared__ uint32_t changed;
    __shared__ uint32_t part[kAddDeepBlock / 64];
    const uint64_t pr = blockIdx.x;
    if (pr >= A.n) return;
    if (pair_class && pair_class[pr] == PAIR_LARGE) return;   // over edge_budget: k_add_merge.hip
    const uint32_t tid = threadIdx.x;
    const uint32_t LA = (uint32_t)A.l_cnt[pr], LB = (uint32_t)B.l_cnt[pr];
    const uint32_t L = LA + LB;
    const uint64_t nA = A.e_cnt[pr], nB = B.e_cnt[pr];
    const uint64_t alo = A.l_off[pr], blo = B.l_off[pr], aeo = A.e_off[pr], beo = B.e_off[pr];
    const uint64_t clo = C.l_off[pr], ceo = C.e_off[pr];
    uint32_t* keep = slab + clo;   // [L]

    for (uint32_t l = tid; l < L; l += kAddDeepBlock) keep[l] = 0;
    __syncthreads();
    // used by edges (encrypt.hpp:78)
    for (uint64_t e = tid; e < nA; e += kAddDeepBlock) {
        const uint32_t lid = meta_layer(A.meta[aeo + e]);
        if (lid < L) keep[lid] = 1;
    }
    for (uint64_t e = tid; e < nB; e += kAddDeepBlock) {
        const uint32_t lid = meta_layer(B.meta[beo + e]) + LA;
        if (lid < L) keep[lid] = 1;
    }
    // transitive closure over PROD parents, parallel sweeps until stable
    for (;;) {
        __syncthreads();
        if (tid == 0) changed = 0;
        __syncthreads();
        for (uint32_t l = tid; l < L; l += kAddDeepBlock) {
            if (!keep[l]) continue;
            const pvac_layer& x = l < LA ? A.layers[alo + l] : B.layers[blo + (l - LA)];
            if (x.rule != 1) continue;
            const uint32_t off = l < LA ? 0u : LA;
            const uint32_t pa = x.pa + off, pb = x.pb + off;
            if (pa < L && !keep[pa]) { keep[pa] = 1; changed = 1; }
            if (pb < L && !keep[pb]) { keep[pb] = 1; changed = 1; }
        }
        __syncthreads();
        if (!changed) break;
    }
    // remap = exclusive count of kept layers, tiles in index order
    uint32_t kept = 0;
    for (uint32_t b0 = 0; b0 < L; b0 += 4u * kAddDeepBlock) {
        const uint32_t l0 = b0 + 4u * tid;
        uint32_t v[4];
        uint32_t local = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            v[k] = l0 + k < L ? keep[l0 + k] : 0u;
            local += v[k];
        }
        uint32_t tot;
        uint32_t run = kept + block_exclusive_scan<kAddDeepBlock>(local, part, tot);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (l0 + k < L) keep[l0 + k] = v[k] ? run : 0xFFFFFFFFu;
            run += v[k];
        }
        kept += tot;
    }
    __syncthreads();
    const bool identity = kept == L;
    // layers
    for (uint32_t l = tid; l < L; l += kAddDeepBlock) {
        const uint32_t to = keep[l];
        if (to == 0xFFFFFFFFu) continue;
        pvac_layer y = l < LA ? A.layers[alo + l] : B.layers[blo + (l - LA)];
        if (l >= LA && y.rule == 1) { y.pa += LA; y.pb += LA; }
        if (!identity && y.rule == 1) {
            y.pa = y.pa < L ? keep[y.pa] : 0xFFFFFFFFu;
            y.pb = y.pb < L ? keep[y.pb] : 0xFFFFFFFFu;
        }
        C.layers[clo + to] = y;
    }
    if (tid == 0) {
        C.l_cnt[pr] = kept;
        C.e_cnt[pr] = nA + nB;
    }
    // edges (concat; B shifted and optionally scaled by p-1)
    const fp pm1{kAll - 1, kM63};
    for (uint64_t e = tid; e < nA + nB; e += kAddDeepBlock) {
        const bool fromB = e >= nA;
        const uint64_t src = fromB ? beo + (e - nA) : aeo + e;
        uint64_t m = fromB ? B.meta[src] : A.meta[src];
        uint64_t wl = fromB ? B.w_lo[src] : A.w_lo[src];
        uint64_t wh = fromB ? B.w_hi[src] : A.w_hi[src];
        uint32_t lid = meta_layer(m) + (fromB ? LA : 0u);
        if (!identity) lid = lid < L ? keep[lid] : 0xFFFFFFFFu;
        m = (m & ~0xFFFFFFFFull) | lid;
        if (fromB && negate_b) {
            const fp r = fp_mul(fp{wl, wh}, pm1);
            wl = r.lo; wh = r.hi;
        }
        C.meta[ceo + e] = m;
        C.w_lo[ceo + e] = wl;
        C.w_hi[ceo + e] = wh;
    }
    // sigma carry: one 16-byte chunk per work item
    if (C.sigma && A.sigma && B.sigma) {
        const uint32_t sw = C.sigma_words;
        const uint64_t chunks_per_edge = sw / 2;
        const uint64_t total = (nA + nB) * chunks_per_edge;
        for (uint64_t c = tid; c < total; c += kAddDeepBlock) {
            const uint64_t e = c / chunks_per_edge, k = c - e * chunks_per_edge;
            const bool fromB = e >= nA;
            const ulonglong2* srcp = fromB ? (const ulonglong2*)(B.sigma + (beo + (e - nA)) * B.sigma_words)
                                           : (const ulonglong2*)(A.sigma + (aeo + e) * A.sigma_words);
            ((ulonglong2*)(C.sigma + (ceo + e) * sw))[k] = srcp[k];
        }
    }
}

}  // namespace

hipError_t launch_ct_mul_large_deep(const mul_large_args& a, int stage, hipStream_t st) {
    if (!a.nl) return hipSuccess;
    if (!a.deep || a.Bm > kBmax || a.max_lay > PVAC_LAYER_LIMIT_MAX || a.any_direct || a.all_iblk || !a.any_dyn)
        return hipErrorInvalidValue;
    const unsigned nl = a.nl;
    const unsigned ge = grid_x(a.max_nA, kLB * 4, 1024), gl = grid_x(a.max_lay, kLB * 2, 1024);
    switch (stage) {
    case 0:
        launch_large_init(a, st);
        break;
    case 1:
        hipLaunchKernelGGL(k_large_lists_deep_hist, dim3(ge, nl), dim3(kLB), 0, st, a);
        hipLaunchKernelGGL(k_large_lists_deep_alloc, dim3(gl, nl), dim3(kLB), 0, st, a);
        hipLaunchKernelGGL(k_large_lists_deep_scatter, dim3(ge, nl), dim3(kLB), 0, st, a);
        break;
    case 2:
        launch_large_products(a, st);
        break;
    case 3:
        hipLaunchKernelGGL(k_large_layers_deep, dim3(nl), dim3(kLBig), 0, st, a);
        hipLaunchKernelGGL(k_large_layers_deep_write, dim3(gl, nl), dim3(kLB), 0, st, a);
        break;
    case 4:
        launch_large_emit(a, st);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_ct_add_deep(const pvac_ct_batch& A, const pvac_ct_batch& B, pvac_ct_batch& C, int negate_b,
                              uint32_t* slab, const uint8_t* pair_class, hipStream_t st) {
    if (!A.n) return hipSuccess;
    if (!slab || A.n > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ct_add_deep, dim3((unsigned)A.n), dim3(kAddDeepBlock), 0, st, A, B, C, negate_b, slab, pair_class);
    return hipGetLastError();
}

}  // namespace pvhip
