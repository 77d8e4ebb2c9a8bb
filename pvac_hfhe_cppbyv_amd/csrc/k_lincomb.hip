// k_lincomb.hip — ct_lincomb: segmented sums of optionally scaled ciphers of one batch in one pass.
//
// The reference's fold acc = ct_add(pk, acc, t_k) (ops/arithmetic.hpp:12-31) does no arithmetic: it
// concatenates, offsets layer ids and PROD parents, and runs compact_layers (ops/encrypt.hpp:73-104).
// For terms inside the Cipher contract and a sum within edge_budget the result is "compact each term
// on its own, then concatenate with offsets", so every term can be placed independently:
//   plan pass  k_lincomb_plan     per term, a lane group: the layers compact_layers keeps, as a 64-bit
//                                 mask (terms of at most 64 layers), and the contract flag
//              k_lincomb_plan_wg  the same for larger terms, one workgroup each, keep table in LDS,
//                                 the remap left in scratch
//              k_lincomb_split, k_lincomb_plan_deep  a term above kLinMaxLayers layers (a context with
//                                 a raised layer limit): the keep table in scratch too, where the remap goes
//              k_lincomb_index    the segment of every term; seg_off's own checks
//              (u64 scans over the terms: layer, edge and kept-layer offsets)
//              k_lincomb_classify per segment: one pass, or the host's fold (over budget, contract)
//              k_lincomb_layout   C's offsets and the copy pass's tile tables
//   copy pass  k_lincomb_layers   one thread per input layer slot
//              k_lincomb_copy     one workgroup per kLinEdgeTile OUTPUT edges (the output is dense, so
//                                 a term of any size is spread over as many workgroups as it fills),
//                                 weights scaled where flagged, then the tile's sigma rows
//              k_lincomb_counts   per segment: l_cnt / e_cnt
#include <algorithm>

#include "common.hpp"
#include "compact_layers.hpp"

namespace pvhip {

namespace {

constexpr int kLinBlock = 256;
constexpr uint32_t kNone = kDropped;   // map_layer: dropped, or not one of the term's layers
constexpr uint32_t kTileTerms = 256;   // terms of an edge tile whose records are staged in LDS

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// A statistic's maximum: the wave's first, then one look at the stored value per wave and an atomic
// only when it is beaten (see k_ct.hip: the stored maximum never decreases, so skipping is exact; a
// look per lane at one address serialises at its L2 channel). Every lane of the wave calls it.
__device__ __forceinline__ void wave_max_if_greater(unsigned int* p, uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63u) == 0 && v > __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMax(p, v);
}

// the last index in [lo, hi) whose entry is <= v (s non-decreasing with s[lo] <= v; any other
// content still stays inside [lo, hi))
__device__ __forceinline__ uint64_t last_le(const uint64_t* s, uint64_t lo, uint64_t hi, uint64_t v) {
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (s[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------- plan pass
// what a group needs of its term before it can touch the term's rows: one dependent round trip
struct term_head {
    uint64_t L, E, xlo, xeo;
    bool ok;   // the term index is one of X's
};

__device__ __forceinline__ term_head load_head(const lincomb_args& a, uint64_t k) {
    term_head h{0, 0, 0, 0, false};
    if (k >= a.n_terms) return h;
    const uint64_t t = a.term[k];
    if (t >= a.X.n) return h;
    h.ok = true;
    h.L = a.X.l_cnt[t];
    h.E = a.X.e_cnt[t];
    h.xlo = a.X.l_off[t];
    h.xeo = a.X.e_off[t];
    return h;
}

__device__ __forceinline__ bool wave_route(const term_head& h) { return h.L <= kLinWaveLayers && h.E <= kLinWaveEdges; }

// One term per group of G lanes (G = 32: two terms per wave, both of at most 32 layers). Lane l holds
// layer l's PROD parents; the closure is compact_layers.hpp's wave form. A dead group (tail, bad index, a term of
// the workgroup route) runs with zero counts, so every group reaches the same shuffles.
template <int G>
__device__ __forceinline__ void plan_term(const lincomb_args& a, uint64_t k, bool live, const term_head& h) {
    const pvac_ct_batch& X = a.X;
    const uint32_t gl = (threadIdx.x & 63u) & (uint32_t)(G - 1);
    const bool wg = !wave_route(h);
    const uint32_t Lw = wg ? 0u : (uint32_t)h.L;   // <= G: the caller picks G from it
    const uint64_t Ew = wg ? 0ull : h.E;
    uint32_t rule = 0, pa = 0, pb = 0;
    if (gl < Lw) {
        const pvac_layer* y = X.layers + h.xlo + gl;
        rule = y->rule;
        pa = y->pa;
        pb = y->pb;
    }
    // layers used by edges (encrypt.hpp:78); an edge beyond the term's own layers is out of contract
    uint64_t used = 0, bad = 0;
#pragma unroll 4
    for (uint64_t e = gl; e < Ew; e += G) {
        const uint32_t lid = meta_layer(X.meta[h.xeo + e]);
        if (lid < Lw) used |= 1ull << lid;
        else bad = 1;
    }
    used = group_or_u64<G>(used);
    // transitive PROD parents (encrypt.hpp:80-88)
    const uint64_t mypm =
        (gl < Lw && rule == 1) ? ((pa < Lw ? 1ull << pa : 0ull) | (pb < Lw ? 1ull << pb : 0ull)) : 0ull;
    const uint64_t keep = group_close<G>(used, mypm, gl);
    // a kept PROD layer whose parent is not one of the term's layers (remap[pa] out of range there)
    if (gl < Lw && ((keep >> gl) & 1ull) && rule == 1 && (pa >= Lw || pb >= Lw)) bad = 1;
    bad = group_or_u64<G>(bad);
    if (live && gl == 0) {
        a.sL[k] = h.L;
        a.sE[k] = h.E;
        a.kraw[k] = wg ? 0ull : ((uint64_t)__popcll(keep) | (bad << 40));
        a.mask[k] = keep;
        a.troute[k] = wg ? 1 : 0;
        if (!h.ok) atomicAdd(&a.stats->n_invalid, 1ull);
        if (wg) a.wg_ids[atomicAdd(&a.stats->n_small, 1ull)] = k;
        if (k == 0) a.sL[a.n_terms] = a.sE[a.n_terms] = a.kraw[a.n_terms] = 0;   // the scans' closing entries
    }
}

__global__ __launch_bounds__(kLinBlock) void k_lincomb_plan(lincomb_args a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t k0 = ((uint64_t)blockIdx.x * (kLinBlock / 64) + wave) * 2;   // the wave's two terms
    // each half of the wave loads the head of its own term; the choice of G needs both
    const uint64_t kh = k0 + (lane >> 5);
    const term_head h = load_head(a, kh);
    const uint32_t Lh = wave_route(h) ? (uint32_t)h.L : 0u;   // layers the term asks of its group
    if (__all(Lh <= 32u)) {
        plan_term<32>(a, kh, kh < a.n_terms, h);
        return;
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {   // one term at a time on all 64 lanes, its head from lane 32 * half
        term_head g;
        g.L = (uint64_t)__shfl((long long)h.L, 32 * half, 64);
        g.E = (uint64_t)__shfl((long long)h.E, 32 * half, 64);
        g.xlo = (uint64_t)__shfl((long long)h.xlo, 32 * half, 64);
        g.xeo = (uint64_t)__shfl((long long)h.xeo, 32 * half, 64);
        g.ok = __shfl((int)h.ok, 32 * half, 64) != 0;
        plan_term<64>(a, k0 + half, k0 + half < a.n_terms, g);
    }
}

// u < n_terms: the segment of term u and the terms' largest counts (sL / sE before their scans);
// u <= n: seg_off's checks (0 first, n_terms last, non-decreasing)
__global__ __launch_bounds__(kLinBlock) void k_lincomb_index(lincomb_args a) {
    const uint64_t u = (uint64_t)blockIdx.x * kLinBlock + threadIdx.x;
    uint32_t ml = 0, me = 0;
    if (u < a.n_terms) {
        const uint64_t s = last_le(a.seg_off, 0, a.n + 1, u);
        a.tseg[u] = (uint32_t)(s < a.n ? s : a.n - 1);
        ml = sat32(a.sL[u]);
        me = sat32(a.sE[u]);
    }
    wave_max_if_greater(&a.stats->max_layers, ml);
    wave_max_if_greater(&a.stats->max_na, me);
    if (u <= a.n) {
        const uint64_t v = a.seg_off[u];
        bool bad = false;
        if (u == 0) bad = v != 0;
        if (u == a.n) bad = bad || v != a.n_terms;
        else bad = bad || v > a.seg_off[u + 1];
        if (bad) atomicAdd(&a.stats->n_invalid, 1ull);
    }
}

// The workgroup route: one term per workgroup, compact_layers.hpp's workgroup form on a keep table in LDS
// (k_ct_add's index checks are the contract flag here). Needs the scanned sL: the term's remap table lies at sL[k].
__global__ __launch_bounds__(kLinBlock) void k_lincomb_plan_wg(lincomb_args a, uint64_t n_wg) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint32_t* keep = (uint32_t*)lds;
    __shared__ uint32_t changed, bad;   // a sweep marked a layer; the term is out of contract
    __shared__ uint32_t part[kLinBlock / 64];
    const pvac_ct_batch& X = a.X;
    const uint32_t tid = threadIdx.x;
    for (uint64_t w = blockIdx.x; w < n_wg; w += gridDim.x) {
        const uint64_t k = a.wg_ids[w];
        const uint64_t t = a.term[k];
        const uint32_t L = (uint32_t)X.l_cnt[t];   // <= kLinMaxLayers (host-checked)
        const uint64_t E = X.e_cnt[t], xeo = X.e_off[t];
        const pvac_layer* lay = X.layers + X.l_off[t];
        for (uint32_t l = tid; l < L; l += kLinBlock) keep[l] = 0;
        if (tid == 0) bad = 0;
        __syncthreads();
        for (uint64_t e = tid; e < E; e += kLinBlock) {
            const uint32_t lid = meta_layer(X.meta[xeo + e]);
            if (lid < L) keep[lid] = 1;
            else bad = 1;
        }
        block_close<kLinBlock>(keep, L, &changed, [&](uint32_t l, uint32_t& rule, uint32_t& pa, uint32_t& pb) {
            rule = lay[l].rule; pa = lay[l].pa; pb = lay[l].pb;
            if (rule == 1 && (pa >= L || pb >= L)) bad = 1;   // a kept PROD layer with a parent beyond the term
        });
        // the remap to scratch; its closing barrier also frees keep[] and bad for the next term
        const uint32_t kept = block_remap<kLinBlock>(keep, a.remap + a.sL[k], L, part);
        if (tid == 0) a.kraw[k] = (uint64_t)kept | ((uint64_t)bad << 40);
    }
}

// A call with a term above kLinMaxLayers: the terms beyond the wave route, split by route. out[0] / out[1]
// count the workgroup / deep-term route's terms, listed (in any order) from out + 2 / out + 2 + n_terms.
__global__ __launch_bounds__(kLinBlock) void k_lincomb_split(lincomb_args a, uint64_t n_wg, uint64_t* out) {
    const uint64_t w = (uint64_t)blockIdx.x * kLinBlock + threadIdx.x;
    if (w >= n_wg) return;
    const uint64_t k = a.wg_ids[w];
    const uint64_t t = a.term[k];
    const bool deep = lincomb_route(a.X.l_cnt[t], a.X.e_cnt[t]) == LIN_ROUTE_DEEP;
    const uint64_t at = atomicAdd((unsigned long long*)out + (deep ? 1 : 0), 1ull);
    out[2 + (deep ? a.n_terms : 0ull) + at] = k;
}

// The deep-term route: k_lincomb_plan_wg with the keep table where the remap goes, in the slab at
// sL[k] (global memory: compact_layers.hpp's contract covers a table there), so nothing is sized by
// the layer count. One workgroup per term, grid-stride over its layers and edge headers; the closure
// is block_close's, monotone, and ends when a sweep of this workgroup marks nothing.
constexpr int kLinDeepBlock = 1024;
__global__ __launch_bounds__(kLinDeepBlock) void k_lincomb_plan_deep(lincomb_args a, const uint64_t* deep_ids,
                                                                      uint64_t n_deep) {
    __shared__ uint32_t changed, bad;
    __shared__ uint32_t part[kLinDeepBlock / 64];
    const pvac_ct_batch& X = a.X;
    const uint32_t tid = threadIdx.x;
    for (uint64_t w = blockIdx.x; w < n_deep; w += gridDim.x) {
        const uint64_t k = deep_ids[w];
        const uint64_t t = a.term[k];
        const uint32_t L = (uint32_t)X.l_cnt[t];   // at most the context's layer limit (host-checked)
        const uint64_t E = X.e_cnt[t], xeo = X.e_off[t];
        const pvac_layer* lay = X.layers + X.l_off[t];
        uint32_t* keep = a.remap + a.sL[k];        // L words of the slab: sL is the scan of the terms' layer counts
        for (uint32_t l = tid; l < L; l += kLinDeepBlock) keep[l] = 0;
        if (tid == 0) bad = 0;
        __syncthreads();
        for (uint64_t e = tid; e < E; e += kLinDeepBlock) {
            const uint32_t lid = meta_layer(X.meta[xeo + e]);
            if (lid < L) keep[lid] = 1;
            else bad = 1;
        }
        block_close<kLinDeepBlock>(keep, L, &changed, [&](uint32_t l, uint32_t& rule, uint32_t& pa, uint32_t& pb) {
            rule = lay[l].rule; pa = lay[l].pa; pb = lay[l].pb;
            if (rule == 1 && (pa >= L || pb >= L)) bad = 1;   // a kept PROD layer with a parent beyond the term
        });
        const uint32_t kept = block_remap<kLinDeepBlock>(keep, keep, L, part);   // its closing barrier frees `bad`
        if (tid == 0) a.kraw[k] = (uint64_t)kept | ((uint64_t)bad << 40);
    }
}

__global__ __launch_bounds__(kLinBlock) void k_lincomb_classify(lincomb_args a) {
    const uint64_t i = (uint64_t)blockIdx.x * kLinBlock + threadIdx.x;
    uint32_t ml = 0, me = 0, mf = 0;
    if (i < a.n) {
        const uint64_t lo = a.seg_off[i], hi = a.seg_off[i + 1];
        if (lo <= hi && hi <= a.n_terms) {   // else counted by k_lincomb_index: the plan fails
            const uint64_t dL = a.sL[hi] - a.sL[lo], dE = a.sE[hi] - a.sE[lo];
            const uint64_t flagged = (a.sK[hi] - a.sK[lo]) >> 40;
            // guard_budget: the prefix sums are monotone, so some step's guard fires exactly when the total does
            const uint32_t cls = dE > a.edge_budget ? LIN_FOLD_BUDGET : flagged ? LIN_FOLD_CONTRACT : LIN_ONE_PASS;
            a.cls[i] = cls;
            ml = sat32(dL);
            me = sat32(dE);
            if (cls != LIN_ONE_PASS) {
                a.fold_ids[atomicAdd(&a.stats->n_large, 1ull)] = i;
                mf = ml;
            }
        }
    }
    wave_max_if_greater(&a.stats->max_prod, ml);
    wave_max_if_greater(&a.stats->max_nb, me);
    wave_max_if_greater(&a.stats->max_buckets, mf);
}

__global__ __launch_bounds__(kLinBlock) void k_lincomb_layout(lincomb_args a, uint64_t total_layers, uint64_t total_edges,
                                                              uint64_t tiles_l, uint64_t tiles_e) {
    const uint64_t u = (uint64_t)blockIdx.x * kLinBlock + threadIdx.x;
    if (u < a.n) {
        const uint64_t lo = a.seg_off[u];
        a.C.l_off[u] = a.sL[lo];
        a.C.e_off[u] = a.sE[lo];
    }
    if (!a.n_terms) return;
    if (u < tiles_l) a.tile_l[u] = (uint32_t)last_le(a.sL, 0, a.n_terms + 1, u * kLinLayerTile);
    if (u == tiles_l) a.tile_l[u] = (uint32_t)(a.n_terms - 1);
    if (u < tiles_e) a.tile_e[u] = (uint32_t)last_le(a.sE, 0, a.n_terms + 1, u * kLinEdgeTile);
    if (u == tiles_e) a.tile_e[u] = (uint32_t)(a.n_terms - 1);
}

// ---------------------------------------------------------------- copy pass
// what an edge or a layer needs of its term
struct term_info {
    uint64_t e0;      // sE[k]: the term's first output edge
    uint64_t src;     // X.e_off[term]
    uint64_t mask;    // wave route: keep mask
    uint64_t rbase;   // sL[k]: the term's first input layer slot and its remap table
    uint64_t s_lo, s_hi;
    uint32_t kbase;   // kept layers of the segment's earlier terms
    uint32_t L;
    uint32_t fl;      // kScaled | kRouteWg | kSkip | kIdentity
    uint32_t seg;
};
enum : uint32_t { kScaled = 1, kRouteWg = 2, kSkip = 4, kIdentity = 8 };

__device__ __forceinline__ term_info load_term(const lincomb_args& a, uint64_t k) {
    term_info f;
    const uint64_t t = a.term[k];
    f.seg = a.tseg[k];
    const uint64_t lo = a.seg_off[f.seg];
    f.e0 = a.sE[k];
    f.src = a.X.e_off[t];
    f.mask = a.mask[k];
    f.rbase = a.sL[k];
    f.L = (uint32_t)(a.sL[k + 1] - f.rbase);
    f.kbase = (uint32_t)((a.sK[k] - a.sK[lo]) & kLinKeptMask);
    const bool scaled = a.scale && (!a.flags || (a.flags[k] & PVAC_TERM_SCALE));
    f.s_lo = scaled ? a.scale[2 * k] : 0ull;
    f.s_hi = scaled ? a.scale[2 * k + 1] : 0ull;
    f.fl = (scaled ? kScaled : 0u) | (a.troute[k] ? kRouteWg : 0u) | (a.cls[f.seg] != LIN_ONE_PASS ? kSkip : 0u) |
           ((a.kraw[k] & kLinKeptMask) == f.L ? kIdentity : 0u);
    return f;
}

// layer `lid` of the term in its output cipher (kNone: dropped, or not one of the term's)
__device__ __forceinline__ uint32_t map_layer(const lincomb_args& a, const term_info& f, uint32_t lid) {
    if (lid >= f.L) return kNone;
    uint32_t to = lid;
    if (!(f.fl & kIdentity)) {
        if (f.fl & kRouteWg) to = a.remap[f.rbase + lid];
        else to = ((f.mask >> lid) & 1ull) ? (uint32_t)__popcll(f.mask & ((1ull << lid) - 1ull)) : kNone;
    }
    return to == kNone ? kNone : to + f.kbase;
}

__global__ __launch_bounds__(kLinBlock) void k_lincomb_layers(lincomb_args a, uint64_t total_layers) {
    const uint64_t j = (uint64_t)blockIdx.x * kLinLayerTile + threadIdx.x;
    if (j >= total_layers) return;
    const uint64_t k = last_le(a.sL, a.tile_l[blockIdx.x], (uint64_t)a.tile_l[blockIdx.x + 1] + 1, j);
    const term_info f = load_term(a, k);
    if (f.fl & kSkip) return;
    const uint32_t l = (uint32_t)(j - f.rbase);
    const uint32_t to = map_layer(a, f, l);
    if (to == kNone) return;
    const uint64_t t = a.term[k];
    pvac_layer y = a.X.layers[a.X.l_off[t] + l];
    if (y.rule == 1) {   // parents inside the term (a kept PROD parent beyond it is the fold route's)
        y.pa = map_layer(a, f, y.pa);
        y.pb = map_layer(a, f, y.pb);
    }
    a.C.layers[a.sL[a.seg_off[f.seg]] + to] = y;
}

__global__ __launch_bounds__(kLinBlock) void k_lincomb_copy(lincomb_args a, uint64_t total_edges, int sigma, int wide) {
    __shared__ term_info ti[kTileTerms];
    const pvac_ct_batch& X = a.X;
    const pvac_ct_batch& C = a.C;
    const uint32_t tid = threadIdx.x;
    const uint64_t j0 = (uint64_t)blockIdx.x * kLinEdgeTile;
    const uint64_t j1 = j0 + kLinEdgeTile < total_edges ? j0 + kLinEdgeTile : total_edges;
    const uint64_t kA = a.tile_e[blockIdx.x], kB = a.tile_e[blockIdx.x + 1];
    const uint32_t nT = (uint32_t)(kB - kA + 1);
    const bool cached = nT <= kTileTerms;   // else (runs of empty terms) every lookup goes to memory
    if (cached) {
        for (uint32_t u = tid; u < nT; u += kLinBlock) ti[u] = load_term(a, kA + u);
        __syncthreads();
    }
    // the term of output edge j, as an index into ti (cached) or a term number
    auto find = [&](uint64_t j) -> uint64_t {
        if (!cached) return last_le(a.sE, kA, kB + 1, j);
        uint32_t lo = 0, hi = nT;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (ti[mid].e0 <= j) lo = mid;
            else hi = mid;
        }
        return lo;
    };
    auto info = [&](uint64_t ref) -> term_info { return cached ? ti[ref] : load_term(a, ref); };

    constexpr int kPer = kLinEdgeTile / kLinBlock;
    uint64_t ref[kPer], m[kPer], wl[kPer], wh[kPer];
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const uint64_t j = j0 + (uint64_t)r * kLinBlock + tid;
        ref[r] = 0; m[r] = 0; wl[r] = 0; wh[r] = 0;
        if (j < j1) {
            ref[r] = find(j);
            uint64_t e0, src;
            if (cached) { e0 = ti[ref[r]].e0; src = ti[ref[r]].src; }
            else { e0 = a.sE[ref[r]]; src = X.e_off[a.term[ref[r]]]; }
            const uint64_t s = src + (j - e0);
            m[r] = X.meta[s];
            wl[r] = X.w_lo[s];
            wh[r] = X.w_hi[s];
        }
    }
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const uint64_t j = j0 + (uint64_t)r * kLinBlock + tid;
        if (j >= j1) continue;
        const term_info f = info(ref[r]);
        if (f.fl & kSkip) continue;
        const uint64_t mo = (m[r] & ~0xFFFFFFFFull) | map_layer(a, f, meta_layer(m[r]));
        uint64_t lo = wl[r], hi = wh[r];
        if (f.fl & kScaled) {   // ct_scale (arithmetic.hpp:33-37), whatever the scale
            const fp q = fp_mul(fp{lo, hi}, fp{f.s_lo, f.s_hi});
            lo = q.lo;
            hi = q.hi;
        }
        __builtin_nontemporal_store((unsigned long long)mo, (unsigned long long*)C.meta + j);
        __builtin_nontemporal_store((unsigned long long)lo, (unsigned long long*)C.w_lo + j);
        __builtin_nontemporal_store((unsigned long long)hi, (unsigned long long*)C.w_hi + j);
    }
    if (!sigma) return;
    // sigma rows by whole waves: 16 bytes per lane, four rows in flight (128-word rows), streamed
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const uint32_t sw = C.sigma_words;
    if (wide) {
        for (uint64_t jb = j0 + wave * 4u; jb < j1; jb += 4u * (kLinBlock / 64)) {
            u64x2 v[4];
            bool on[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint64_t j = jb + q;
                on[q] = j < j1;
                if (!on[q]) continue;
                const term_info f = info(find(j));
                on[q] = !(f.fl & kSkip);
                if (on[q]) v[q] = __builtin_nontemporal_load((const u64x2*)(X.sigma + (f.src + (j - f.e0)) * 128u) + lane);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (on[q]) __builtin_nontemporal_store(v[q], (u64x2*)(C.sigma + (jb + q) * 128u) + lane);
        }
        return;
    }
    for (uint64_t j = j0 + wave; j < j1; j += kLinBlock / 64) {
        const term_info f = info(find(j));
        if (f.fl & kSkip) continue;
        const uint64_t* s = X.sigma + (f.src + (j - f.e0)) * sw;
        for (uint32_t w = lane; w < sw; w += 64) C.sigma[j * sw + w] = s[w];
    }
}

__global__ __launch_bounds__(kLinBlock) void k_lincomb_counts(lincomb_args a) {
    const uint64_t i = (uint64_t)blockIdx.x * kLinBlock + threadIdx.x;
    if (i >= a.n || a.cls[i] != LIN_ONE_PASS) return;
    const uint64_t lo = a.seg_off[i], hi = a.seg_off[i + 1];
    a.C.l_cnt[i] = (a.sK[hi] - a.sK[lo]) & kLinKeptMask;
    a.C.e_cnt[i] = a.sE[hi] - a.sE[lo];
}

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + kLinBlock - 1) / kLinBlock); }

}  // namespace

// ==================================================================== launch wrappers
hipError_t launch_lincomb_plan(const lincomb_args& a, hipStream_t st) {
    if (a.n_terms)
        hipLaunchKernelGGL(k_lincomb_plan, dim3((unsigned)((a.n_terms + 2 * (kLinBlock / 64) - 1) / (2 * (kLinBlock / 64)))),
                           dim3(kLinBlock), 0, st, a);
    const uint64_t m = a.n_terms > a.n + 1 ? a.n_terms : a.n + 1;
    hipLaunchKernelGGL(k_lincomb_index, dim3(blocks_for(m)), dim3(kLinBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_lincomb_plan_wg(const lincomb_args& a, uint64_t n_wg, uint32_t max_layers, hipStream_t st) {
    if (!n_wg) return hipSuccess;
    if (max_layers > kLinMaxLayers) return hipErrorInvalidValue;
    const size_t lds = ((size_t)max_layers * 4 + 15) & ~(size_t)15;
    hipLaunchKernelGGL(k_lincomb_plan_wg, dim3((unsigned)(n_wg < 2048 ? n_wg : 2048)), dim3(kLinBlock), lds, st, a, n_wg);
    return hipGetLastError();
}

hipError_t launch_lincomb_split(const lincomb_args& a, uint64_t n_wg, uint64_t* out, hipStream_t st) {
    if (!n_wg) return hipSuccess;
    hipLaunchKernelGGL(k_lincomb_split, dim3(blocks_for(n_wg)), dim3(kLinBlock), 0, st, a, n_wg, out);
    return hipGetLastError();
}

hipError_t launch_lincomb_plan_deep(const lincomb_args& a, const uint64_t* deep_ids, uint64_t n_deep, hipStream_t st) {
    if (!n_deep) return hipSuccess;
    hipLaunchKernelGGL(k_lincomb_plan_deep, dim3((unsigned)(n_deep < 2048 ? n_deep : 2048)), dim3(kLinDeepBlock), 0, st, a,
                       deep_ids, n_deep);
    return hipGetLastError();
}

hipError_t launch_lincomb_classify(const lincomb_args& a, hipStream_t st) {
    if (!a.n) return hipSuccess;
    hipLaunchKernelGGL(k_lincomb_classify, dim3(blocks_for(a.n)), dim3(kLinBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_lincomb_layout(const lincomb_args& a, uint64_t total_layers, uint64_t total_edges, hipStream_t st) {
    const uint64_t tl = a.n_terms ? (total_layers + kLinLayerTile - 1) / kLinLayerTile : 0;
    const uint64_t te = a.n_terms ? (total_edges + kLinEdgeTile - 1) / kLinEdgeTile : 0;
    uint64_t m = a.n;
    if (a.n_terms) m = std::max(m, std::max(tl, te) + 1);
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_lincomb_layout, dim3(blocks_for(m)), dim3(kLinBlock), 0, st, a, total_layers, total_edges, tl, te);
    return hipGetLastError();
}

hipError_t launch_lincomb_copy(const lincomb_args& a, uint64_t total_layers, uint64_t total_edges, hipStream_t st) {
    if (!a.n) return hipSuccess;
    if (a.n_terms && total_layers)
        hipLaunchKernelGGL(k_lincomb_layers, dim3((unsigned)((total_layers + kLinLayerTile - 1) / kLinLayerTile)),
                           dim3(kLinBlock), 0, st, a, total_layers);
    if (a.n_terms && total_edges) {
        const int sigma = a.X.sigma && a.C.sigma;
        const int wide = sigma && a.X.sigma_words == 128 && a.C.sigma_words == 128 && ((uintptr_t)a.X.sigma & 15u) == 0 &&
                         ((uintptr_t)a.C.sigma & 15u) == 0;
        hipLaunchKernelGGL(k_lincomb_copy, dim3((unsigned)((total_edges + kLinEdgeTile - 1) / kLinEdgeTile)),
                           dim3(kLinBlock), 0, st, a, total_edges, sigma, wide);
    }
    hipLaunchKernelGGL(k_lincomb_counts, dim3(blocks_for(a.n)), dim3(kLinBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace pvhip
