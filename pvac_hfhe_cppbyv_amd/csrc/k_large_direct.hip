// k_large_direct.hip — the direct mode of the general ct_mul path (large_desc::direct; the launch
// sequence is in k_mul_large.hip): k_large_count_la and k_large_scan_direct fix every output
// position from key presence before any multiply, k_large_products_direct multiplies on the matrix
// cores and writes C's records at those positions, k_large_direct_redo lists the pairs that need the
// host's redo after all.
#include "k_large_mx.hpp"

#ifdef PVAC_DIR_STAMPS   // diagnostic build only: the stamping kernels' accumulators (DSTAMP, k_large.hpp)
__device__ unsigned long long g_dir_stamps[24];
extern "C" int pvac_hip_diag_dir_stamps(unsigned long long* host, int reset) {
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_dir_stamps), sizeof(g_dir_stamps)) != hipSuccess) return -5;
    if (reset) {
        unsigned long long z[24] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_dir_stamps), z, sizeof(z)) != hipSuccess) return -5;
    }
    return 0;
}
#endif

namespace pvhip {

namespace {

typedef unsigned int u2v __attribute__((ext_vector_type(2)));

// k_large_count_la's per-A-layer output, held in registers so that its global stores can be issued
// after the next layer's staging has consumed its loads (a wave's vmcnt counts stores and loads in
// one FIFO: stores issued between a load and its use made that use wait for them)
constexpr uint32_t kPendCells = 3;   // dense cells per thread held (2 B <= 3 x 256 for B <= 384)
struct cnt_pend {
    uint32_t i[kPendCells], w[kPendCells], k[kPendCells];   // A edge, list word, list slot + 1 (0: none)
    ulonglong2 m[kPendCells];
    uint32_t n;        // the layer's list length
    uint32_t used;     // product layers (bit k: B layer k) with a key, from this thread's keys
};

// iblk_layer's counts and masks for a direct pair, as the A layer's writer list: the A edges whose
// ranges hold keys, wl[k] = A edge i | its idx << 21 and imask[k] = (P mask, M mask) in any order
// (slots from an LDS counter), so that k_large_products_direct reads one contiguous list per A layer.
// k_large_lists zeroed the count bytes; only ranges with keys store theirs. Cells beyond kPendCells per
// thread store at once. Barriers inside; every thread calls it.
template <int BS>
__device__ void cnt_layer_list(uint8_t* plds, uint32_t Bm, uint32_t nB, uint64_t nb_m, uint32_t nk, const uint32_t* recs,
                               cnt_pend& p, uint8_t* icnt, uint32_t* wl, ulonglong2* imask) {
    unsigned long long* M1 = (unsigned long long*)plds;
    unsigned long long* M2 = M1 + 2u * Bm;
    const uint32_t* tt = (const uint32_t*)(plds + cnt_tt_off(Bm));
    uint32_t* wn = (uint32_t*)(plds + cnt_len_off(Bm));   // after stage_tt's dup word
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < 4u * Bm; k += BS) M1[k] = 0ull;
    if (tid == 0) *wn = 0;
    __syncthreads();
    for (uint32_t q = tid; q < nk; q += BS) {   // (no shared buckets in a direct pair)
        const uint32_t v = recs[q];
        if (!v) continue;
        const uint32_t dd = v & 0xFFFu, j = (v >> 12) & 63u, e = (v >> 18) & 3u;
        if (e & 1u) atomicOr(&M1[dd], 1ull << j);
        if (e & 2u) atomicOr(&M2[dd], 1ull << j);
    }
    __syncthreads();
    // cell dd: its list word and slot + 1 (0: no range with keys), its masks
    auto cell = [&](uint32_t dd, uint32_t& i, uint32_t& w, ulonglong2& mk) -> uint32_t {
        if (dd >= 2u * Bm) return 0u;
        const uint32_t ch = dd >= Bm ? 1u : 0u;
        const uint32_t te = tt[dd + ch * Bm];   // tt slot ch 2B + idx
        if (te == kInf) return 0u;
        const unsigned long long x1 = M1[dd], x2 = M2[dd];
        if (!(x1 | x2)) return 0u;
        uint32_t j;
        i = div_small(te, nB, nb_m, j);
        w = i | (dd - ch * Bm) << 21;
        mk = make_ulonglong2(x1, x2);
        return atomicAdd(wn, 1u) + 1u;
    };
#pragma unroll
    for (uint32_t v = 0; v < kPendCells; ++v) p.k[v] = cell(tid + v * BS, p.i[v], p.w[v], p.m[v]);
    for (uint32_t dd = tid + kPendCells * BS; dd < 2u * Bm; dd += BS) {   // B > 384 only
        uint32_t i, w;
        ulonglong2 mk;
        const uint32_t k = cell(dd, i, w, mk);
        if (!k) continue;
        icnt[i] = (uint8_t)(__popcll(mk.x) + __popcll(mk.y));   // <= 128
        wl[k - 1u] = w;
        imask[k - 1u] = mk;
    }
    __syncthreads();   // the next A layer's staging overwrites M1 / M2, tt and recs
    p.n = *wn;
}

__device__ __forceinline__ void cnt_flush(const cnt_pend& p, uint8_t* icnt, uint32_t* wl, ulonglong2* imask,
                                          uint32_t* wln) {
#pragma unroll
    for (uint32_t u = 0; u < kPendCells; ++u) {
        if (!p.k[u]) continue;
        icnt[p.i[u]] = (uint8_t)(__popcll(p.m[u].x) + __popcll(p.m[u].y));
        wl[p.k[u] - 1u] = p.w[u];
        imask[p.k[u] - 1u] = p.m[u];
    }
    if (threadIdx.x == 0) *wln = p.n;
}
// Which keys emit, and in which order, follows from key PRESENCE alone when no key's products cancel:
// a P (M) cell emits iff some product lands in it (arithmetic.hpp:96-101 with sums assumed != 0).
// So the per-A-edge counts and masks of iblk_layer can be built before any multiply, the counts
// scanned into offsets, and the products kernel can write C's edge records at their positions from
// its epilogue: no per-key sums, first-insert times or key records go through HBM, and the range
// writer that gathered them is not needed. A key whose sum turns out to be 0 sends the pair to the
// host's redo (exact path), as the fresh kernel does.

// the dense side's first-insert shares only (no digits): tt[2][2B] as mx_stage_dense lays them out,
// at cnt_tt_off (cnt_layer_list reads them there), from the cells in the direct pair's A ids; false
// when the layer has duplicate (idx, ch) edges
template <int BS>
__device__ bool stage_tt(uint8_t* lds, uint32_t Bm, const layer_src& D, uint32_t tmul, const uint32_t (&pre)[4]) {
    uint32_t* tt = (uint32_t*)(lds + cnt_tt_off(Bm));
    uint32_t* dup = (uint32_t*)(lds + cnt_dup_off(Bm));
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < 4 * Bm; k += BS) tt[k] = kInf;
    if (tid == 0) *dup = 0;
    __syncthreads();
    for (uint32_t k0 = tid; k0 < D.n; k0 += 4u * BS) {   // four edges per round (the first: loaded ahead)
        uint32_t e[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const uint32_t k = k0 + (uint32_t)v * BS;
            e[v] = k0 == tid ? pre[v] : D.ids[k < D.n ? k : 0u];   // A edge | dense cell << 21 (k_large_lists)
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            if (k0 + (uint32_t)v * BS >= D.n) break;
            const uint32_t cell = e[v] >> 21, ch = cell >= Bm ? 1u : 0u;
            const uint32_t sl = cell + ch * Bm;   // slot ch 2B + idx
            const uint32_t te = (e[v] & 0x1FFFFFu) * tmul;
            if (atomicCAS(&tt[sl], kInf, te) != kInf) *dup = 1;   // (the claim of mx_stage_dense)
            else tt[sl + Bm] = te;
        }
    }
    __syncthreads();
    return *dup == 0;
}

// Pass 1 of a direct pair, one workgroup per (pair, la_per_wg A layers) like k_large_products_la:
// per A layer, every key (r, B layer) gets its first-insert time and its P / M presence from the
// dense shares and the B layers' edges, one record per key (the products kernel's iblk record),
// then iblk_layer's counts and masks; product-layer used flags for compact_layers. A layer the
// matrix-core mode cannot take (duplicate edges, fewer than kLargeDenseMin edges) fails the pair
// (cnt[kCntIFail]): k_large_scan_direct sends it to the host's redo.
// resident workgroups per CU k_large_count_la is compiled for: 6 (<= 80 VGPRs, no spills) against
// 5 (81 VGPRs unconstrained): cfg-4 chain 195 K against 188-190 K ct_mul/s on one stream; 7 spills
constexpr int kCntMinBlocks = 6;
template <int BS>
__global__ __launch_bounds__(BS, kCntMinBlocks) void k_large_count_la(mul_large_args g) {
    extern __shared__ __attribute__((aligned(16))) uint8_t plds[];
    const large_desc d = g.desc[g.sel[blockIdx.y]];   // registers (the kernel's stores could alias it)
    if (!d.direct) return;
    uint32_t* S = g.scratch;
    uint32_t* cnt = S + d.o_cnt;
    const uint32_t LA = d.LA, LB = d.LB, Bm = g.Bm, nB = d.nB;
    const uint32_t tid = threadIdx.x;
    const uint32_t i0 = blockIdx.x * g.la_per_wg;
    // The prologue's loads in dependency levels, each level's loads issued together (the A and B
    // chains are independent): 1 the pair's counters, its B layer ids, the first A layer id, B's
    // edge offset; 2 the layers' list ranges; 3 the id lists; 4 B's edge metas. (Issued in program
    // order the chains took seven dependent round trips per workgroup.) Reads past a short list
    // stay inside the pair's scratch and are not used.
    const uint32_t c2 = cnt[kCntInvalid], cf = cnt[kCntIFail], c0 = cnt[kCntNeA], c1 = cnt[kCntNeB];
    uint32_t lbv[kLaMaxLB];
#pragma unroll
    for (uint32_t k = 0; k < kLaMaxLB; ++k) lbv[k] = S[d.o_neB + k];
    uint32_t la_c = S[d.o_neA + min(i0, LA - 1u)];
    const uint64_t beo = g.B.e_off[d.pair];
    if (c2 || cf) return;
    const uint32_t neA = c0, neB = min(c1, kLaMaxLB);
    if (i0 >= neA) return;
    const uint32_t i1 = min(neA, i0 + g.la_per_wg);
    // level 2
    uint32_t nbv[kLaMaxLB], bst[kLaMaxLB];
#pragma unroll
    for (uint32_t k = 0; k < kLaMaxLB; ++k) {
        const uint32_t lb = k < neB ? lbv[k] : 0u;
        lbv[k] = lb;
        bst[k] = S[d.o_lstB + lb];
        nbv[k] = k < neB ? S[d.o_lstB + LB + lb] : 0u;   // <= kIblkMaxSparse (k_large_lists failed the pair otherwise)
    }
    uint32_t st_c = S[d.o_lstA + la_c], n_c = S[d.o_lstA + LA + la_c];
    const uint64_t mbj = tid < nB ? g.B.meta[beo + tid] : 0ull;   // bjt below
    // level 3 (A as a dense chain image: its ids are the 32-bit words of its meta region, k_large_lists)
    const bool aimg = g.A_img && g.A_img[d.pair];
    const uint32_t* idsA = aimg ? (const uint32_t*)(g.A.meta + g.A.e_off[d.pair]) : S + d.o_lstA + 2u * LA;
    const uint32_t* idsB = S + d.o_lstB + 2u * LB;
    uint32_t pre[4];
    auto load_ids = [&](uint32_t st, uint32_t n) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const uint32_t k = tid + (uint32_t)v * BS;
            pre[v] = idsA[st + (k < n ? k : 0u)];
        }
    };
    load_ids(st_c, n_c);
    uint32_t eb[kLaMaxLB];
#pragma unroll
    for (uint32_t k = 0; k < kLaMaxLB; ++k) eb[k] = k < neB ? idsB[bst[k] + (tid < nbv[k] ? tid : 0u)] : 0u;
    uint32_t la_n = i0 + 1u < i1 ? S[d.o_neA + i0 + 1u] : 0u;
    // level 4: B layers as per-edge (P slot offset, M slot offset, j, 1), padded to a multiple of 4
    // with (0, 0, INF, 0), as mx_stage_sparse computes them
    uint4* sp = (uint4*)(plds + g.lds_task);                          // [kLaMaxLB][kMxMaxSparse]
    uint32_t* bjt = (uint32_t*)(sp + kLaMaxLB * kMxMaxSparse);        // [64] B edge j: idx | ch << 16
    uint32_t* recs = bjt + 64;                                        // [kLaMaxLB][B]
    uint64_t mbk[kLaMaxLB];
#pragma unroll
    for (uint32_t k = 0; k < kLaMaxLB; ++k) mbk[k] = k < neB ? g.B.meta[beo + eb[k]] : 0ull;
#pragma unroll
    for (uint32_t k = 0; k < kLaMaxLB; ++k) {
        if (k < neB && tid < ((nbv[k] + 3u) & ~3u) && nbv[k] <= kMxMaxSparse) {
            uint4 v = make_uint4(0, 0, kInf, 0);
            if (tid < nbv[k]) {
                const uint32_t sidx = meta_idx(mbk[k]), sch = meta_ch(mbk[k]);
                v = make_uint4(sch * 2u * Bm + Bm - sidx, (sch ^ 1u) * 2u * Bm + Bm - sidx, eb[k], 1);
            }
            sp[k * kMxMaxSparse + tid] = v;
        }
    }
    if (tid < nB) bjt[tid] = meta_idx(mbj) | meta_ch(mbj) << 16;   // published by stage_tt's barriers
    const uint32_t* tt = (const uint32_t*)(plds + cnt_tt_off(Bm));
#ifdef PVAC_DIR_STAMPS
    unsigned long long st_acc[4] = {0, 0, 0, 0}, t_prev = dir_stamp();
#endif
    // the previous layer's outputs, stored after this layer's staging (cnt_pend)
    cnt_pend pend;
    uint32_t pend_la = kInf, pend_base = 0;
    auto flush = [&]() {
        if (pend_la == kInf) return;   // workgroup-uniform
        cnt_flush(pend, (uint8_t*)(S + d.o_icnt), S + d.o_wle + pend_base, (ulonglong2*)(S + d.o_imask) + pend_base,
                  S + d.o_wln + pend_la);
        // product layers with a key: compact_layers keeps them (benign race: every writer stores 1)
#pragma unroll
        for (uint32_t k = 0; k < kLaMaxLB; ++k)
            if ((pend.used >> k) & 1u) S[d.o_used + (LA + LB) + pend_la * LB + lbv[k]] = 1;
        pend_la = kInf;
    };
    for (uint32_t i = i0; i < i1; ++i) {
        DSTAMP(0);
        const uint32_t la = late(la_c);
        const layer_src srcA{&g.A, 0, idsA + late(st_c), late(n_c)};
        bool ok = srcA.n >= kLargeDenseMin;
#pragma unroll
        for (uint32_t k = 0; k < kLaMaxLB; ++k) ok &= k >= neB || (nbv[k] <= kMxMaxSparse && nbv[k] <= srcA.n);
        if (!ok) {   // workgroup-uniform: this A layer's tasks would not all run on the matrix cores
            if (tid == 0) atomicExch(&cnt[kCntIFail], 1u);
            return;
        }
        if (!stage_tt<BS>(plds, Bm, srcA, nB, pre)) {
            if (tid == 0) atomicExch(&cnt[kCntIFail], 1u);
            return;
        }
        DSTAMP(1);
        const uint32_t lx = late(la_n);
        uint32_t st_n = 0, n_n = 0;
        if (i + 1u < i1) {   // workgroup-uniform
            st_n = S[d.o_lstA + lx];
            n_n = S[d.o_lstA + LA + lx];
        }
        flush();   // the previous layer's stores, behind this layer's loads
        uint32_t usedm = 0;
        for (uint32_t q = tid; q < neB * Bm; q += BS) {
            const uint32_t k = q / Bm, r = q - k * Bm;
            const uint4* e = sp + k * kMxMaxSparse;
            uint32_t tmin = kInf, pp = 0, pm = 0;
            // four sparse edges per step (padded lists): their LDS reads in flight together
            for (uint32_t x = 0; x < nbv[k]; x += 4) {
                uint4 in[4];
                uint32_t tp[4], tm[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) in[u] = e[x + u];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    tp[u] = tt[in[u].x + r];
                    tm[u] = tt[in[u].y + r];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    pp |= tp[u] != kInf ? in[u].w : 0u;
                    pm |= tm[u] != kInf ? in[u].w : 0u;
                    tmin = min(tmin, min(__builtin_elementwise_add_sat(tp[u], in[u].z),
                                         __builtin_elementwise_add_sat(tm[u], in[u].z)));
                }
            }
            uint32_t rv = 0;
            if (tmin != kInf) {
                const uint32_t eb = pp | pm << 1;
                // no shared buckets in a direct pair (the host's slots_share_bucket check)
                uint32_t j;
                const uint32_t ia = div_small(tmin, nB, d.nb_m, j);
                const uint32_t ij = bjt[j] & 0xFFFFu;
                const uint32_t xx = r >= ij ? r - ij : r + Bm - ij;
                const uint32_t dd = tt[xx] == ia * nB ? xx : Bm + xx;
                rv = dd | j << 12 | eb << 18 | kRecKey;
                usedm |= 1u << k;
            }
            recs[k * Bm + r] = rv;
        }
        __syncthreads();
        DSTAMP(2);
        uint32_t la_n2 = 0;
        if (i + 1u < i1) {
            load_ids(late(st_n), late(n_n));
            if (i + 2u < i1) la_n2 = S[d.o_neA + i + 2u];
        }
        const uint32_t lbase = late(st_c);   // the layer's list slice: as its edge ids
        cnt_layer_list<BS>(plds, Bm, nB, d.nb_m, neB * Bm, recs, pend, (uint8_t*)(S + d.o_icnt), S + d.o_wle + lbase,
                           (ulonglong2*)(S + d.o_imask) + lbase);
        pend.used = usedm;
        pend_la = la;
        pend_base = lbase;
        DSTAMP(3);
#ifdef PVAC_DIR_STAMPS
        if (tid == 0) atomicAdd(&g_dir_stamps[13], (unsigned long long)pend.n);
#endif
        la_c = lx;
        st_c = st_n;
        n_c = n_n;
        la_n = la_n2;
    }
    flush();
#ifdef PVAC_DIR_STAMPS
    if (tid == 0) {
        for (int p = 0; p < 4; ++p) atomicAdd(&g_dir_stamps[8 + p], st_acc[p]);
        atomicAdd(&g_dir_stamps[12], (unsigned long long)(i1 - i0));
    }
#endif
}

// count bytes of a direct pair's A edges (4 per word): their sum, and the sum over the bytes of a
// 32-edge group at positions above b (the word holding positions lo .. lo + 3)
__device__ __forceinline__ uint32_t byte_sum(uint32_t x) { return __builtin_amdgcn_sad_u8(x, 0u, 0u); }
__device__ __forceinline__ uint32_t byte_sum(const uint4& x) {
    return __builtin_amdgcn_sad_u8(x.x, 0u, __builtin_amdgcn_sad_u8(x.y, 0u, __builtin_amdgcn_sad_u8(x.z, 0u, byte_sum(x.w))));
}
__device__ __forceinline__ uint32_t bytes_above(uint32_t x, uint32_t lo, uint32_t b) {
    const uint32_t m = b < lo ? 0xFFFFFFFFu : b >= lo + 3u ? 0u : 0xFFFFFFFFu << (8u * (b - lo + 1u));
    return byte_sum(x & m);
}
// an A edge's exclusive suffix offset: its group's offset plus the counts of the group's later edges
__device__ __forceinline__ uint32_t dir_edge_off(const uint4* c8, const uint32_t* wo, uint32_t e) {
    const uint32_t gi = e >> 5, b = e & 31u;
    const uint4 a = c8[2u * gi], c = c8[2u * gi + 1u];
    return wo[gi] + bytes_above(a.x, 0u, b) + bytes_above(a.y, 4u, b) + bytes_above(a.z, 8u, b) +
           bytes_above(a.w, 12u, b) + bytes_above(c.x, 16u, b) + bytes_above(c.y, 20u, b) + bytes_above(c.z, 24u, b) +
           bytes_above(c.w, 28u, b);
}

// Pass 2 of a direct pair, one workgroup per pair: the total, the guard_budget decision, and the
// per-A-edge count bytes turned into exclusive suffix offsets per 32-edge group (an edge's own
// offset adds its group's later bytes: dir_edge_off). A pair with shared buckets, a fallback or
// the canonical order is not direct after all: it goes to the host's redo.
__global__ __launch_bounds__(kLBig) void k_large_scan_direct(mul_large_args g) {
    __shared__ uint32_t part[kLBig / 64];
    const large_desc& d = g.desc[blockIdx.x];
    if (!d.direct) return;
    uint32_t* S = g.scratch;
    uint32_t* cnt = S + d.o_cnt;
    if (cnt[kCntInvalid]) return;
    const int tid = threadIdx.x;
    const uint4* c8 = (const uint4*)(S + d.o_icnt);   // count bytes, two uint4 per group of 32 A edges
    uint32_t* wo = S + d.o_iwo;
    const uint32_t ng = (d.nA + 31u) >> 5;
    // one pass: the groups' suffix offsets are written while the total accumulates; a pair that is
    // not direct after all (checked after the pass) is redone, so offsets written for it are never read
    if (cnt[kCntIFail] || cnt[kCntIShared] || (g.flags & PVAC_MUL_ORDER_CANONICAL) != 0) {
        if (tid == 0) {
            cnt[kCntRedo] = 1;
            g.pair_status[d.pair] = kPairRedo;
        }
        return;
    }
    uint32_t run0 = 0;
    for (uint32_t base = 0; base < ng; base += 4u * kLBig) {
        const uint32_t r0 = base + 4u * (uint32_t)tid;
        uint4 x[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // loads first
            const uint32_t r = r0 + (uint32_t)k, w = ng - 1u - r;
            x[2 * k] = r < ng ? c8[2u * w] : make_uint4(0u, 0u, 0u, 0u);
            x[2 * k + 1] = r < ng ? c8[2u * w + 1u] : make_uint4(0u, 0u, 0u, 0u);
        }
        uint32_t v[4];
        uint32_t local = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = byte_sum(x[2 * k]) + byte_sum(x[2 * k + 1]);
            local += v[k];
        }
        uint32_t tot;
        uint32_t run = run0 + block_exclusive_scan<kLBig>(local, part, tot);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t r = r0 + (uint32_t)k;
            if (r < ng) wo[ng - 1u - r] = run;
            run += v[k];
        }
        run0 += tot;
    }
    const uint32_t total = run0;
    if (total > g.edge_budget) {   // guard_budget's canonical order: the general path (redo)
        if (tid == 0) {
            cnt[kCntRedo] = 1;
            g.pair_status[d.pair] = kPairRedo;
        }
        return;
    }
    if (tid == 0) {
        cnt[kCntTotal] = total;
        cnt[kCntCanonical] = 0;
        cnt[kCntDirect] = 1;
        // a chain step writes C as a dense image when every cell of every product layer (la, lb) with
        // edges on both sides holds a key (and the hash positions fit the 21-bit ids the next step's
        // lists carry)
        cnt[kCntImg] = g.C_img && !g.salt_pos && (uint64_t)total == (uint64_t)cnt[kCntNeA] * cnt[kCntNeB] * 2u * g.Bm &&
                               total < (1u << 21)
                           ? 1u
                           : 0u;
        g.C.e_cnt[d.pair] = total;
        g.pair_status[d.pair] = 0;
    }
}

// direct pairs handed to the redo (not direct after all, or a key whose products cancel): onto the
// redo list the host re-runs on the full layout (ct_mul_exec's redo step)
__global__ __launch_bounds__(64) void k_large_direct_redo(mul_large_args g) {
    const uint32_t q = blockIdx.x * 64u + threadIdx.x;
    if (q >= g.nl) return;
    const large_desc& d = g.desc[q];
    if (!d.direct) return;
    const uint32_t* cnt = g.scratch + d.o_cnt;
    if (cnt[kCntInvalid]) return;
    if (!cnt[kCntRedo]) {   // finished here: its C is a dense image when the image writer ran
        if (g.C_img && cnt[kCntDirect] && cnt[kCntImg]) {
            g.C_img[d.pair] = 1u;
            if (g.img_count) atomicAdd(g.img_count, 1ull);
        }
        return;
    }
    g.pair_status[d.pair] = kPairRedo;
    g.redo_ids[atomicAdd(g.redo_cnt, 1u)] = d.pair;
}

// Pass 3 of a direct pair (after k_large_scan_direct and the layers pass), one workgroup per
// (pair, la_per_wg A layers) like k_large_products_la. Per A layer: the matrix-core products of every
// B layer with each row's folded P / M sums staged in LDS by key slot (no first-insert times: the
// order is already in the counts and masks of k_large_count_la), then a range writer: the A layer's
// ranges (its A edges with keys, positions [off(i), off(i) + cnt(i)) of the output) are walked like
// k_large_write_ranges walks all of them, each position resolved to its key (j DESC, P before M) and
// its value read from LDS, so C's records are stored range by range, coalesced, with no per-key
// scratch in HBM. A staged value of 0 at a present cell (products that cancel) flags the pair for
// the host's redo.
//
// LDS: dig1 [2][B] uint4 (one copy per channel: slot (r - idx) mod B with a wrap, 32 B per index) |
// per B layer: prec | pinf (kMxSparseBytes) | bjt [64] | stg [neB][B][2] (16 B per cell): dir_lds_bytes
// (common.hpp; the host sizes the direct mode by it)

// the dense side (an A layer) as digits, one copy per channel (k_large_count_la checked for
// duplicate cells). Barriers inside; every thread calls it.
// slab: kInf, or (A held as a dense chain image) the layer's first edge slot: list entry k's weight
// sits at slab + k instead of at its hash-order edge (a contiguous read instead of a gather)
template <int BS>
__device__ void dir_stage_dense(uint4* dig, uint32_t Bm, const layer_src& D, uint32_t slab) {
    constexpr uint32_t kV = 3;   // a dense A layer (<= 2 B = 674 edges) in one round of loads
    const uint32_t tid = threadIdx.x;
    uint32_t c[kV];
    uint64_t lo[kV], hi[kV];
    auto load = [&](uint32_t k0) {   // direct pairs' A ids: A edge | dense cell << 21 (k_large_lists)
#pragma unroll
        for (uint32_t v = 0; v < kV; ++v) {
            const uint32_t k = k0 + v * BS;
            const uint32_t kc = k < D.n ? k : 0u;   // D.n >= kLargeDenseMin
            const uint32_t id = D.ids[kc];
            c[v] = id >> 21;
            const uint32_t e = slab != kInf ? slab + kc : (id & 0x1FFFFFu);
            lo[v] = D.X->w_lo[D.eo + e];
            hi[v] = D.X->w_hi[D.eo + e];
        }
    };
    auto put = [&](uint32_t k0) {
#pragma unroll
        for (uint32_t v = 0; v < kV; ++v) {
            if (k0 + v * BS >= D.n) break;
            uint64_t dl, dh;
            // an image's weights are the previous step's folded sums, canonical already
            fp_digits8(slab != kInf ? fp{lo[v], hi[v]} : fp_canon(lo[v], hi[v]), dl, dh);
            dig[c[v]] = make_uint4((uint32_t)dl, (uint32_t)(dl >> 32), (uint32_t)dh, (uint32_t)(dh >> 32));
        }
    };
    load(tid);   // in flight across the zero fill and its barrier
    for (uint32_t k = tid; k < 2 * Bm; k += BS) dig[k] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    put(tid);
    for (uint32_t k0 = tid + kV * BS; k0 < D.n; k0 += kV * BS) {
        load(k0);
        put(k0);
    }
    __syncthreads();
}

// a B layer as the MFMA sparse side (prec as mx_stage_sparse) with pinf = (B - idx, P table base,
// M table base) for the one-copy dense table; no first-insert shares. Thread k writes edge k.
__device__ __forceinline__ void dir_stage_sparse(uint4* prec, uint4* pinf, uint32_t Bm, const layer_src& Sd, uint32_t k) {
    const uint32_t nks = (Sd.n + 1u) >> 1;
    if (k >= 2u * nks) return;
    uint4 mid = make_uint4(0, 0, 0, 0);
    uint4 inf = make_uint4(0, 0, Bm, 0);   // padding edge: zero digits
    if (k < Sd.n) {
        const edge_rec x = load_edge(Sd, k);
        mid = mx_rev_digits(x);
        const uint32_t sidx = meta_idx(x.meta), sch = meta_ch(x.meta);
        // pinf for the one-copy dense table, no first-insert share (mx_stage_sparse differs here)
        inf = make_uint4(Bm - sidx, sch * Bm, (sch ^ 1u) * Bm, 0);
    }
    mx_put_prec(prec, k, mid);
    pinf[k] = inf;
}

// one task's products, each row's P (half 0) / M (half 1) sum into stg[(r) 2 + h]
// (the k-steps' sparse-edge offsets are read from LDS per block: held in registers for every block they
// cost 177 instead of 187 VALU per block, but 21 spill ops: 428-429 K against 430-431 K)
template <int BS, int NKS>
__device__ void dir_rows_n(const uint4* dig, const uint4* prec, const uint4* pinf, uint32_t Bm, ulonglong2* stg) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t h = lane >> 5, n = lane & 31u;
    mx_v4 frag[NKS];
    mx_load_frags<NKS>(prec, h, n, frag);
    const uint32_t nblk = (Bm + 31u) >> 5;
    for (uint32_t blk = wave; blk < nblk; blk += BS / 64) {
        const uint32_t r = blk * 32u + n;
        const bool live = r < Bm;
        const uint32_t rr = live ? r : 0u;
        mx_v16 aP{}, aM{};
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
            const uint4 in = pinf[2u * (uint32_t)s + h];
            uint32_t x = rr + in.x;   // (r - idx) mod B
            x = min(x, x - Bm);
            const uint4 dp = dig[in.y + x], dm = dig[in.z + x];
            aP = __builtin_amdgcn_mfma_i32_32x32x32_i8(frag[s], mx_v4{(int)dp.x, (int)dp.y, (int)dp.z, (int)dp.w}, aP, 0, 0, 0);
            aM = __builtin_amdgcn_mfma_i32_32x32x32_i8(frag[s], mx_v4{(int)dm.x, (int)dm.y, (int)dm.z, (int)dm.w}, aM, 0, 0, 0);
        }
        int64_t paw, pbw, maw, mbw;
        mx_groups(aP, paw, pbw);
        mx_groups(aM, maw, mbw);
        const int64_t ra = shfl_xor64(h ? paw : maw, 32), rb = shfl_xor64(h ? pbw : mbw, 32);
        const fp v = mx_fold(h ? ra : paw, h ? maw : ra, h ? rb : pbw, h ? mbw : rb);
        if (live) stg[2u * r + h] = make_ulonglong2(v.lo, v.hi);
    }
}

template <int BS>
__device__ void dir_rows(const uint4* dig, const uint4* prec, const uint4* pinf, uint32_t ns, uint32_t Bm, ulonglong2* stg) {
    mx_for_ks(ns, [](auto ks, auto... a) { dir_rows_n<BS, decltype(ks)::value>(a...); }, dig, prec, pinf, Bm, stg);
}

// cache policy bits of the products kernel's record stores. Streaming (2) was measured against the
// default (0) on the cfg-4 chain: HBM writes 84.4 against 70.8 GB per 4096 inputs (lines leave L2
// before their neighbours' records fill them, then go out again), reads 47.2 against 58.5, time equal
constexpr int kDirStoreAux = 0;
template <int BS>
__global__ __launch_bounds__(BS, kLaMinBlocks) void k_large_products_direct(mul_large_args g) {
    extern __shared__ __attribute__((aligned(16))) uint8_t plds[];
    // a register copy of the descriptor: C's stores could alias it, so field reads through the
    // reference were reloaded from memory (a dependent round trip each) after every store
    const large_desc d = g.desc[g.sel[blockIdx.y]];
    if (!d.direct) return;
    uint32_t* S = g.scratch;
    uint32_t* cnt = S + d.o_cnt;
    if (cnt[kCntInvalid] || !cnt[kCntDirect]) return;
    const uint32_t neA = cnt[kCntNeA], neB = min(cnt[kCntNeB], g.dir_lb);   // the host sized the LDS for dir_lb B layers
    const uint32_t i0 = blockIdx.x * g.la_per_wg;
    if (i0 >= neA) return;
    const uint32_t LA = d.LA, LB = d.LB, Bm = g.Bm, nB = d.nB;
    static_assert(BS <= 256, "dir_lds_base holds the writer's per-entry words for 256 entries");
    const uint32_t tid = threadIdx.x;
#ifdef PVAC_DIR_STAMPS
    unsigned long long st_acc[9] = {}, t_prev = dir_stamp();
#endif
    uint4* dig = (uint4*)plds;
    uint8_t* sreg = plds + dir_lds_base(Bm);                           // per B layer: prec | pinf
    uint32_t* bjt = (uint32_t*)(sreg + g.dir_lb * kMxSparseBytes);     // B edge j: idx | k << 12 | lb << 16
    ulonglong2* stg = (ulonglong2*)(bjt + 64);                         // [k][B][2]
    uint32_t lbv[kLaMaxLB], nbv[kLaMaxLB];
#pragma unroll
    for (uint32_t k = 0; k < kLaMaxLB; ++k) {
        lbv[k] = 0;
        nbv[k] = 0;
        if (k < neB) {
            const uint32_t lb = S[d.o_neB + k];
            const layer_src srcB = side_layer(&g.B, g.B.e_off[d.pair], S, d.o_lstB, LB, lb);
            lbv[k] = lb;
            nbv[k] = srcB.n;   // <= kMxMaxSparse: k_large_count_la checked
            uint4* prec = (uint4*)(sreg + k * kMxSparseBytes);
            dir_stage_sparse(prec, prec + 3u * kMxMaxSparse, Bm, srcB, tid);
        }
    }
    const uint64_t beo = g.B.e_off[d.pair], aeo = g.A.e_off[d.pair], ceo = g.C.e_off[d.pair];
    if (tid < nB) {   // published by the dense staging's barriers
        const uint32_t lb = meta_layer(g.B.meta[beo + tid]);
        uint32_t kk = 0;
#pragma unroll
        for (uint32_t k = 0; k < kLaMaxLB; ++k)
            if (k < neB && lbv[k] == lb) kk = k;
        bjt[tid] = meta_idx(g.B.meta[beo + tid]) | kk << 12 | lb << 16;
    }
    const uint4* c8 = (const uint4*)(S + d.o_icnt);   // count bytes (k_large_count_la)
    const uint32_t* wo = S + d.o_iwo;                 // group offsets (k_large_scan_direct)
    const ulonglong2* wlm = (const ulonglong2*)(S + d.o_imask);   // writer lists (k_large_count_la)
    const uint32_t* wle = S + d.o_wle;
    const uint32_t* remap = S + d.o_used;  // k_large_layers left the remap here (k_large_layers ran before)
    // C's records by buffer stores: one 32-bit offset for the three arrays
    const __amdgpu_buffer_rsrc_t rmeta = __builtin_amdgcn_make_buffer_rsrc(g.C.meta + ceo, 0, 0x7FFFFFF8, 0x00020000);
    const __amdgpu_buffer_rsrc_t rlo = __builtin_amdgcn_make_buffer_rsrc(g.C.w_lo + ceo, 0, 0x7FFFFFF8, 0x00020000);
    const __amdgpu_buffer_rsrc_t rhi = __builtin_amdgcn_make_buffer_rsrc(g.C.w_hi + ceo, 0, 0x7FFFFFF8, 0x00020000);
    const uint32_t i1 = min(neA, i0 + g.la_per_wg);
    const bool aimg = g.A_img && g.A_img[d.pair];   // A as dense images (k_large_lists made its lists the slabs)
    const bool cimg = cnt[kCntImg] != 0;             // C as dense images (k_large_scan_direct)
    // image slabs: C's kept product layers are exactly those with keys, last in C's layer order and in
    // (la, lb) order, one slab of 2B cells each: C layer lid's slab starts at (lid - nbase) 2B
    const uint32_t nbase = cimg ? (uint32_t)g.C.l_cnt[d.pair] - cnt[kCntNeA] * cnt[kCntNeB] : 0u;   // k_large_layers set l_cnt
    // layer headers one layer ahead: the next layer's id loads during this layer's staging, its
    // list range and writer-list length during this layer's writer
    uint32_t la = S[d.o_neA + i0];
    uint32_t a_start = S[d.o_lstA + la], a_n = S[d.o_lstA + LA + la], a_nw = S[d.o_wln + la];
    for (uint32_t ia = i0; ia < i1; ++ia) {
        const layer_src srcA{&g.A, aeo, (aimg ? (const uint32_t*)(g.A.meta + aeo) : S + d.o_lstA + 2u * LA) + a_start, a_n};
        uint32_t lid[kLaMaxLB];
#pragma unroll
        for (uint32_t k = 0; k < kLaMaxLB; ++k) lid[k] = k < neB ? remap[LA + LB + la * LB + lbv[k]] : 0u;
        const uint32_t la_nx = ia + 1u < i1 ? S[d.o_neA + ia + 1u] : 0u;
        DSTAMP(0);
        dir_stage_dense<BS>(dig, Bm, srcA, aimg ? a_start : kInf);   // barriers inside (they also publish the B staging)
        DSTAMP(1);
        for (uint32_t k = 0; k < neB; ++k) {
            const uint4* prec = (const uint4*)(sreg + k * kMxSparseBytes);
            dir_rows<BS>(dig, prec, prec + 3u * kMxMaxSparse, nbv[k], Bm, stg + 2u * Bm * k);
        }
        __syncthreads();
        DSTAMP(2);
        // writer: the A layer's list (its A edges with keys, contiguous; one offset gather each), a
        // round of up to BS list entries at a time. Each entry's thread expands its range's keys in
        // emit order (j DESC, P before M at one j) into okey[excl + kk] (the dead digit table), then
        // every thread takes output slots q = tid, tid + BS, ... of the round: balanced across the
        // waves, stores coalesced within each range, no search.
        const uint32_t lx = late(la_nx);
        uint32_t st_nx = 0, n_nx = 0, nw_nx = 0;
        if (ia + 1u < i1) {   // workgroup-uniform
            st_nx = S[d.o_lstA + lx];
            n_nx = S[d.o_lstA + LA + lx];
            nw_nx = S[d.o_wln + lx];
        }
        const uint32_t lbase = a_start, nw = a_nw;
        uint16_t* okey = (uint16_t*)dig;                       // [<= 8 B] j | ch << 6 | entry << 7
        uint32_t* obase = (uint32_t*)(plds + 16u * Bm);        // [BS] position base: off(i) - excl
        uint32_t* oidx = obase + BS;                           // [BS] the entry's A idx
        uint32_t* oexc = oidx + BS;                            // [BS] the entry's first slot in okey
        ulonglong2* omk = (ulonglong2*)(oexc + BS);            // [BS] the entry's P / M masks
        uint32_t* part = (uint32_t*)(omk + BS);                // [BS / 64] scan partials
        const uint32_t lane = tid & 63u, wave = tid >> 6;
        if (cimg) {
            // dense image writer (a chain step whose C the next step reads): C layer lid (a product
            // layer with keys) owns the 2B slots from (lid - nbase) 2B, cell c = ch B + r at slot + c:
            // 32-bit word s of C's meta region = hash-order position | c << 21 (the next step's list id),
            // the weights in cell order. One wave per writer-list entry, one lane per B edge j: key (j, P) sits after
            // the entry's keys of larger j, (j, M) right after (j, P). With at most two B layers (chain
            // steps) the positions go to an LDS table by cell (the dead okey region, 8 B x 2B) and every
            // store is coalesced; otherwise each key's meta is stored where it is found.
            const bool ptab_ok = neB <= 2u;   // workgroup-uniform
            uint32_t* ptab = (uint32_t*)plds;   // [k][2B] position of cell c of staged B layer k
            // lane j's B edge (the same for every entry): its idx, staged layer and position row
            const uint32_t bjl = bjt[lane];
            const uint32_t kbl = (bjl >> 12) & 15u, idxl = bjl & 0xFFFu;
            uint32_t* const ptl = ptab + kbl * 2u * Bm;
            for (uint32_t b0 = 0; b0 < nw; b0 += BS) {   // workgroup-uniform
                const uint32_t kq = b0 + tid;
                const bool lv = kq < nw;
                const uint32_t we = lv ? wle[lbase + kq] : 0u;
                const ulonglong2 mk = lv ? wlm[lbase + kq] : make_ulonglong2(0ull, 0ull);
                obase[tid] = lv ? dir_edge_off(c8, wo, we & 0x1FFFFFu) : 0u;
                oidx[tid] = we >> 21;
                omk[tid] = make_ulonglong2(mk.x & ~(1ull << 63), mk.y);
                __syncthreads();
                DSTAMP(4);
                const uint32_t ne = min(nw - b0, (uint32_t)BS);
                for (uint32_t l = wave; l < ne; l += BS / 64) {   // wave-uniform
                    const ulonglong2 m2 = omk[l];
                    const uint32_t hp = (uint32_t)(m2.x >> lane) & 1u, hm = (uint32_t)(m2.y >> lane) & 1u;
                    if (!(hp | hm)) continue;
                    const uint32_t above =
                        lane == 63u ? 0u : (uint32_t)__popcll(m2.x >> (lane + 1u)) + (uint32_t)__popcll(m2.y >> (lane + 1u));
                    const uint32_t pos = obase[l] + above;
                    const uint32_t r = mod_small(oidx[l] + idxl, Bm);
                    if (ptab_ok) {
                        if (hp) ptl[r] = pos;
                        if (hm) ptl[Bm + r] = pos + hp;
                        continue;
                    }
                    const uint32_t kb = kbl;
                    const uint32_t lidk = kb == 0 ? lid[0] : kb == 1 ? lid[1] : kb == 2 ? lid[2] : lid[3];
                    const uint32_t sbase = (lidk - nbase) * 2u * Bm;   // < 2^21 (k_large_scan_direct)
                    if (hp) {
                        const ulonglong2 w = stg[(kb * Bm + r) * 2u];
                        if ((w.x | w.y) == 0ull) cnt[kCntRedo] = 1u;   // a present cell whose products cancel
                        __builtin_amdgcn_raw_buffer_store_b32(pos | r << 21, rmeta, (sbase + r) * 4u, 0, kDirStoreAux);
                    }
                    if (hm) {
                        const ulonglong2 w = stg[(kb * Bm + r) * 2u + 1u];
                        if ((w.x | w.y) == 0ull) cnt[kCntRedo] = 1u;
                        __builtin_amdgcn_raw_buffer_store_b32((pos + hp) | (Bm + r) << 21, rmeta, (sbase + Bm + r) * 4u, 0,
                                                              kDirStoreAux);
                    }
                }
                if (b0 + BS < nw) __syncthreads();   // the next round rewrites obase / oidx / omk
            }
            if (ptab_ok) __syncthreads();   // every position in the table
            DSTAMP(5);
#pragma unroll
            for (uint32_t k = 0; k < kLaMaxLB; ++k) {   // the weights of every cell, coalesced
                if (k >= neB) break;
                const uint32_t sbase = (lid[k] - nbase) * 2u * Bm;
                for (uint32_t c = tid; c < 2u * Bm; c += BS) {
                    const uint32_t ch = c >= Bm ? 1u : 0u, r = c - ch * Bm;
                    const ulonglong2 w = stg[(k * Bm + r) * 2u + ch];
                    const uint32_t bo = (sbase + c) * 8u;
                    if (ptab_ok) {   // every cell is a key (the image is dense)
                        if ((w.x | w.y) == 0ull) cnt[kCntRedo] = 1u;   // a present cell whose products cancel
                        __builtin_amdgcn_raw_buffer_store_b32(ptab[k * 2u * Bm + c] | c << 21, rmeta, (sbase + c) * 4u, 0,
                                                              kDirStoreAux);
                    }
                    __builtin_amdgcn_raw_buffer_store_b64(u2v{(uint32_t)w.x, (uint32_t)(w.x >> 32)}, rlo, bo, 0, kDirStoreAux);
                    __builtin_amdgcn_raw_buffer_store_b64(u2v{(uint32_t)w.y, (uint32_t)(w.y >> 32)}, rhi, bo, 0, kDirStoreAux);
                }
            }
            DSTAMP(8);
        }
        for (uint32_t b0 = 0; b0 < nw && !cimg; b0 += BS) {   // workgroup-uniform
            const uint32_t kq = b0 + tid;
            const bool lv = kq < nw;
            const uint32_t we = lv ? wle[lbase + kq] : 0u;
            const ulonglong2 mk = lv ? wlm[lbase + kq] : make_ulonglong2(0ull, 0ull);
            const uint32_t e = we & 0x1FFFFFu;
            const uint32_t oi = lv ? dir_edge_off(c8, wo, e) : 0u;
            const uint64_t mp = mk.x & ~(1ull << 63), mm = mk.y;   // bit 63: a shared bucket (such pairs are redone)
            uint32_t T;
            const uint32_t excl = block_exclusive_scan<BS>((uint32_t)__popcll(mp) + (uint32_t)__popcll(mm), part, T);
            obase[tid] = oi - excl;
            oidx[tid] = we >> 21;
            oexc[tid] = excl;
            omk[tid] = make_ulonglong2(mp, mm);
            __syncthreads();
            DSTAMP(6);
            // key expansion, one wave per entry and one lane per B edge j: the range's keys in emit
            // order (j DESC, P before M at one j), so key (j, P) sits at the keys above j
            const uint32_t ne = min(nw - b0, (uint32_t)BS);
            for (uint32_t l = wave; l < ne; l += BS / 64) {   // wave-uniform
                const ulonglong2 m2 = omk[l];
                const uint32_t x0 = oexc[l];
                const uint32_t hp = (uint32_t)(m2.x >> lane) & 1u, hm = (uint32_t)(m2.y >> lane) & 1u;
                const uint32_t above = lane == 63u ? 0u
                                                   : (uint32_t)__popcll(m2.x >> (lane + 1u)) + (uint32_t)__popcll(m2.y >> (lane + 1u));
                if (hp) okey[x0 + above] = (uint16_t)(lane | l << 7);
                if (hm) okey[x0 + above + hp] = (uint16_t)(lane | 64u | l << 7);
            }
            __syncthreads();
            DSTAMP(7);
            for (uint32_t q = tid; q < T; q += BS) {
                const uint32_t v = okey[q];
                const uint32_t l = v >> 7, jj = v & 63u, ch = (v >> 6) & 1u;
                const uint32_t bj = bjt[jj];
                const uint32_t kb = (bj >> 12) & 15u;
                const uint32_t r = mod_small(oidx[l] + (bj & 0xFFFu), Bm);
                const ulonglong2 w = stg[(kb * Bm + r) * 2u + ch];
                if ((w.x | w.y) == 0ull) cnt[kCntRedo] = 1u;   // a present cell whose products cancel
                const uint32_t lidk = kb == 0 ? lid[0] : kb == 1 ? lid[1] : kb == 2 ? lid[2] : lid[3];
                const uint32_t pos = obase[l] + q;
                const uint64_t mv = make_meta(lidk, r, ch);
                const uint32_t bo = pos * 8u;   // < 2^31: the host caps a direct pair at 2^21 A edges
                __builtin_amdgcn_raw_buffer_store_b64(u2v{(uint32_t)mv, (uint32_t)(mv >> 32)}, rmeta, bo, 0, kDirStoreAux);
                __builtin_amdgcn_raw_buffer_store_b64(u2v{(uint32_t)w.x, (uint32_t)(w.x >> 32)}, rlo, bo, 0, kDirStoreAux);
                __builtin_amdgcn_raw_buffer_store_b64(u2v{(uint32_t)w.y, (uint32_t)(w.y >> 32)}, rhi, bo, 0, kDirStoreAux);
                if (g.salt_pos) g.salt_pos[ceo + pos] = pos;
            }
            if (b0 + BS < nw) __syncthreads();   // the next round rewrites okey / obase
        }
        __syncthreads();   // the next A layer's staging overwrites dig and stg
        DSTAMP(3);
        la = lx;
        a_start = late(st_nx);
        a_n = late(n_nx);
        a_nw = late(nw_nx);
    }
#ifdef PVAC_DIR_STAMPS
    if (tid == 0) {
        for (int p = 0; p < 4; ++p) atomicAdd(&g_dir_stamps[p], st_acc[p]);
        for (int p = 4; p < 9; ++p) atomicAdd(&g_dir_stamps[12 + p], st_acc[p]);   // writer parts: [16, 21)
        atomicAdd(&g_dir_stamps[4], (unsigned long long)(i1 - i0));
        atomicAdd(&g_dir_stamps[5], 1ull);
    }
#endif
}

}  // namespace

// direct pairs, before their k_large_layers pass: presence counts, then offsets
void launch_large_direct_count(mul_large_args& b, hipStream_t st) {
    b.lds_task = cnt_lds_bytes(b.Bm);
    const dim3 grid((unsigned)b.max_la_wg, b.n_la);
    hipLaunchKernelGGL((k_large_count_la<kLPX>), grid, dim3(kLPX),
                       (size_t)b.lds_task + kLaMaxLB * kMxMaxSparse * 16u + kIblkBjtBytes + kLaMaxLB * 4u * b.Bm, st, b);
    hipLaunchKernelGGL(k_large_scan_direct, dim3(b.nl), dim3(kLBig), 0, st, b);
}

// direct pairs, after their k_large_layers pass: products straight to C, then the redo list
void launch_large_direct_products(const mul_large_args& b, hipStream_t st) {
    const dim3 grid((unsigned)b.max_la_wg, b.n_la);
    hipLaunchKernelGGL((k_large_products_direct<kLPX>), grid, dim3(kLPX), (size_t)dir_lds_bytes(b.Bm, b.dir_lb), st, b);
    hipLaunchKernelGGL(k_large_direct_redo, dim3((b.nl + 63) / 64), dim3(64), 0, st, b);
}

}  // namespace pvhip
