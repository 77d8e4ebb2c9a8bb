// k_large_deep.hip — the general ct_mul path for DEEP ciphers: pairs whose layer count is beyond the
// LDS tables of k_large_lists / k_large_layers (Lc = |A.L| + |B.L| + |A.L||B.L| > kLargeLayersMax).
// Nothing here sizes an LDS array by a layer count: the per-layer tables live in the pair's global
// scratch, layer ids are full 32-bit words. (ct_add / ct_sub of deep ciphers: k_ct_add_deep, k_ct.hip.)
//
// A deep pair runs the dynamic route of k_mul_large.hip (bucket table + chains, per-key sums)
// with its lists and layers stages replaced:
//   lists  : the histogram and the cursors of the per-layer edge lists live in used[0, |A.L| + |B.L|):
//            k_large_init zeroed it, and nothing reads it before the layers stage, which starts from
//            used[l >= |A.L| + |B.L|] alone. Three grid-stride kernels over the pair's edges, layers
//            and edges again (hist, alloc, scatter); the scatter pass reads the metas again (no packed
//            copy of a layer id). The lists' contents are what k_large_lists leaves for a pair that is
//            neither an image nor direct: lstA / lstB (start, count), neA / neB, idsA / idsB, four
//            counters; orders inside a list are arrival orders there too.
//   layers : one workgroup per pair runs compact_layers.hpp's closure and remap in place in used[],
//            and a grid-stride kernel writes the kept records.
#include "compact_layers.hpp"
#include "k_large.hpp"

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
// One workgroup per pair (encrypt.hpp:73-104), in place in used[0, Lc): keep flags = product layers
// with emitted edges (the products stage's marks), closed over PROD parents; then flag -> remap.
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
    block_close<kLBig>(used, Lc, &changed, [&](uint32_t l, uint32_t& rule, uint32_t& pa, uint32_t& pb) {
        layer_parents(g, alo, blo, LA, LB, l, rule, pa, pb);
    });
    const uint32_t total = block_remap<kLBig>(used, used, Lc, part);
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
    const uint32_t LA = d.LA, LB = d.LB, Lc = (uint32_t)d.Lc;
    const uint64_t alo = g.A.l_off[pr], blo = g.B.l_off[pr], clo = g.C.l_off[pr];
    const uint32_t* remap = S + d.o_used;
    const bool identity = S[d.o_cnt + kCntKept] == Lc;
    const uint64_t stride = (uint64_t)gridDim.x * kLB;
    for (uint64_t lw = (uint64_t)blockIdx.x * kLB + threadIdx.x; lw < Lc; lw += stride) {
        const uint32_t l = (uint32_t)lw;
        const uint32_t to = remap[l];
        if (to == kDropped) continue;
        pvac_layer y = layer_record(g, alo, blo, clo, LA, LB, l);
        remap_parents(y, remap, Lc, identity);
        g.C.layers[clo + to] = y;
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

}  // namespace pvhip
