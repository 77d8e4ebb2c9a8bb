// k_large_products.hip — the products stage of the general ct_mul path (k_mul_large.hip) for every
// pair that is not direct: one (la, lb) task per workgroup (k_large_products), A-layer-major with
// the per-A-edge emit order of iblk pairs (k_large_products_la), and the column-mode tasks that
// kernel defers (k_large_products_defer). The direct pairs' products are in k_large_direct.hip.
#include "k_large_mx.hpp"

#include <algorithm>

namespace pvhip {

namespace {

// ---------------------------------------------------------------- products (one task per WG)
constexpr uint32_t kChunk = 128;         // sparse-side edges staged per round (chain steps: ~20)
// one product per sparse edge goes into each lane's P and M column sets between col26_norm calls
static_assert(kChunk <= kCol26MaxProducts, "col26 columns overflow: normalise more often");

// dense mode: dl4[2][2B] (limbs 0-3, 16 B) | dx[2][2B] (limb 4, first-insert share) | sl4[kChunk]
//             (16 B) | sl1[kChunk] | sinf[kChunk] | sid[kChunk] | dup. Per channel the B dense slots
//             are stored twice (x and x + B), so lane r finds slot (r - sidx) mod B at r + B - sidx:
//             no wrap test, and the sparse edge's part of the address is wave-uniform (SALU)
constexpr uint32_t kDenseFixed = 96u, kDenseChunk = 28u;
// scatter   : acc[2B x 3] (u64) | tk[B]
__host__ __device__ inline uint32_t prod_lds_bytes(uint32_t Bm) {
    const uint32_t dense = al16(kDenseFixed * Bm) + kDenseChunk * kChunk + 16u;
    const uint32_t scat = 48u * Bm + 4u * Bm;
    return dense > scat ? dense : scat;
}

// the dense side of a task into dig / tt. Every thread calls it; barriers inside; false
// (workgroup-uniform) when the layer holds duplicate (idx, ch) edges. (stage_tt in k_large_direct.hip
// claims tt slots the same way; one helper for both moved the second tt store ahead of the digit
// stores here and changed k_large_products' and k_large_products_la's instruction counts.)
template <int BS>
__device__ bool mx_stage_dense(uint8_t* lds, uint32_t Bm, const layer_src& D, uint32_t tmul) {
    uint4* dig = (uint4*)lds;
    uint32_t* tt = (uint32_t*)(lds + mx_tt_off(Bm));
    uint32_t* dup = (uint32_t*)(lds + mx_dup_off(Bm));
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < 4 * Bm; k += BS) {
        dig[k] = make_uint4(0, 0, 0, 0);
        tt[k] = kInf;
    }
    if (tid == 0) *dup = 0;
    __syncthreads();
    for (uint32_t k0 = tid; k0 < D.n; k0 += 2u * BS) {   // two edges per round, loads first
        edge_rec x[2];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const uint32_t k = k0 + (uint32_t)v * BS;
            x[v] = load_edge(D, k < D.n ? k : 0u);
        }
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            if (k0 + (uint32_t)v * BS >= D.n) break;
            const uint32_t sl = meta_ch(x[v].meta) * 2u * Bm + meta_idx(x[v].meta);
            const uint32_t te = x[v].e * tmul;   // the dense side's share of t = i |B.E| + j
            if (atomicCAS(&tt[sl], kInf, te) != kInf) {
                *dup = 1;
            } else {
                uint64_t dl, dh;
                fp_digits8(fp_canon(x[v].lo, x[v].hi), dl, dh);
                dig[sl] = dig[sl + Bm] = make_uint4((uint32_t)dl, (uint32_t)(dl >> 32), (uint32_t)dh, (uint32_t)(dh >> 32));
                tt[sl + Bm] = te;
            }
        }
    }
    __syncthreads();
    return *dup == 0;
}

// the sparse side of a task (n <= kMxMaxSparse edges) into prec / pinf; thread k writes edge k
// (an odd count gets a zero padding edge). No barrier.
__device__ __forceinline__ void mx_stage_sparse(uint4* prec, uint4* pinf, uint32_t Bm, const layer_src& Sd, uint32_t smul,
                                                uint32_t k) {
    const uint32_t nks = (Sd.n + 1u) >> 1;
    if (k >= 2u * nks) return;
    uint4 mid = make_uint4(0, 0, 0, 0);
    uint4 inf = make_uint4(Bm, Bm, kInf, 0);   // padding edge: zero digits, time never smaller, w = 0
    if (k < Sd.n) {
        const edge_rec x = load_edge(Sd, k);
        mid = mx_rev_digits(x);
        const uint32_t sidx = meta_idx(x.meta), sch = meta_ch(x.meta);
        // pinf for the two-copy dense table with first-insert shares (dir_stage_sparse differs here):
        // dense slot of output row r: P (dense channel == sparse channel), M (the other)
        inf = make_uint4(sch * 2u * Bm + Bm - sidx, (sch ^ 1u) * 2u * Bm + Bm - sidx, x.e * smul, 0);
    }
    mx_put_prec(prec, k, mid);
    pinf[k] = inf;
}

// where a task's results go: dense key-slot arrays of the pair
struct task_out {
    uint32_t* tkey;
    uint32_t* info;
    ulonglong2* sums;
    const uint32_t* ghead;              // static bucket groups (nullptr: dynamic chains)
    unsigned long long* bpack;          // bucket-leader block marks
    // iblk (k_large_products_la): per output row of this B layer, the key's record (kRecKey) for iblk_layer
    uint32_t* recs = nullptr;
    const uint32_t* bjt = nullptr;      // B edge j: idx | ch << 16
    uint32_t nB = 0;
    uint64_t nb_m = 0;
};

// the products of one staged task on the matrix cores: each wave takes blocks of 32 output rows
// (both channels), writes tkey / info / sums and marks lone bucket leaders. No barrier; returns
// whether any of this thread's keys emits.
// NKS = k-steps of two sparse edges, a compile-time count: the k-step loop is straight-line code,
// so every k-step's LDS reads can be issued ahead of the MFMAs (a runtime guard per k-step made
// each one a basic block of its own: two dependent LDS round trips per k-step)
template <int BS, int NKS>
__device__ bool mx_blocks_n(const uint8_t* lds, const uint4* prec, const uint4* pinf, uint32_t Bm, uint64_t slot0,
                            const task_out& o) {
    const uint4* dig = (const uint4*)lds;
    const uint32_t* tt = (const uint32_t*)(lds + mx_tt_off(Bm));
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t h = lane >> 5, n = lane & 31u;
    bool any = false;
    mx_v4 frag[NKS];
    mx_load_frags<NKS>(prec, h, n, frag);
    const uint32_t nblk = (Bm + 31u) >> 5;
    MXMARK(1);
    for (uint32_t blk = wave; blk < nblk; blk += BS / 64) {
        MXMARK(2);
        const uint32_t r = blk * 32u + n;
        const bool live = r < Bm;
        const uint32_t rr = live ? r : 0u;
        mx_v16 aP{}, aM{};
        uint32_t tmin = kInf;
        uint32_t rq = rr;   // opaque copy: without it the k-steps' table reads are scheduled differently
        asm volatile("" : "+v"(rq));   // (the measured code has it)
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
            const uint4 in = pinf[2u * (uint32_t)s + h];
            const uint4 dp = dig[in.x + rq], dm = dig[in.y + rq];
            const uint32_t tp = tt[in.x + rq], tm = tt[in.y + rq];
            aP = __builtin_amdgcn_mfma_i32_32x32x32_i8(frag[s], mx_v4{(int)dp.x, (int)dp.y, (int)dp.z, (int)dp.w}, aP, 0, 0, 0);
            aM = __builtin_amdgcn_mfma_i32_32x32x32_i8(frag[s], mx_v4{(int)dm.x, (int)dm.y, (int)dm.z, (int)dm.w}, aM, 0, 0, 0);
            tmin = min(tmin, min(__builtin_elementwise_add_sat(tp, in.z), __builtin_elementwise_add_sat(tm, in.z)));
        }
        MXMARK(3);
        // half 0 folds row r's P sum, half 1 its M sum; each needs the other half's two words
        int64_t paw, pbw, maw, mbw;
        mx_groups(aP, paw, pbw);
        mx_groups(aM, maw, mbw);
        const int64_t ra = shfl_xor64(h ? paw : maw, 32), rb = shfl_xor64(h ? pbw : mbw, 32);
        MXMARK(4);
        const fp v = mx_fold(h ? ra : paw, h ? maw : ra, h ? rb : pbw, h ? mbw : rb);
        MXMARK(5);
        const uint32_t nz = fp_nonzero(v) ? 1u : 0u;
        const uint32_t nzo = (uint32_t)__shfl_xor((int)nz, 32);
        const uint32_t eb = h ? (nzo | nz << 1) : (nz | nzo << 1);
        tmin = min(tmin, (uint32_t)__shfl_xor((int)tmin, 32));
        if (live) {
            const uint64_t s = slot0 + r;
            if (h == 0) o.tkey[s] = tmin;
            if (tmin != kInf) {
                o.sums[2 * s + h] = make_ulonglong2(v.lo, v.hi);
                if (h == 0) {
                    o.info[s] = eb;
                    if (eb && o.bpack && o.ghead && o.ghead[s] == 0u) leader_mark(o.bpack, tmin, __popc(eb));
                }
                any |= eb != 0;
            }
            if (o.recs && h == 0) {   // iblk: the key's A edge (dense slot) and B edge j
                uint32_t rv = 0;
                const bool shared = tmin != kInf && o.ghead && o.ghead[s] != 0u;
                if (tmin != kInf && (eb || shared)) {
                    uint32_t j;
                    const uint32_t i = div_small(tmin, o.nB, o.nb_m, j);
                    const uint32_t ij = o.bjt[j] & 0xFFFFu;
                    const uint32_t x = r >= ij ? r - ij : r + Bm - ij;
                    const uint32_t dd = tt[x] == i * o.nB ? x : Bm + x;
                    rv = dd | j << 12 | eb << 18 | (shared ? kRecShared : 0u) | kRecKey;
                }
                o.recs[r] = rv;
            }
        }
    }
    return any;
}

template <int BS>
__device__ bool mx_blocks(const uint8_t* lds, const uint4* prec, const uint4* pinf, uint32_t ns, uint32_t Bm, uint64_t slot0,
                          const task_out& o) {
    bool any = false;   // ns = 0, no products: the slots keep their initial time
    mx_for_ks(ns, [&](auto ks) { any = mx_blocks_n<BS, decltype(ks)::value>(lds, prec, pinf, Bm, slot0, o); });
    return any;
}

// One (la, lb) task: the matrix-core dense mode when MX and the sparse side is small, else the
// column-accumulator dense mode (when col26_ok), else (sparse x sparse, duplicate edges) the
// scatter mode. Every thread of the workgroup calls it (barriers inside); LDS from plds,
// prod_lds_bytes(B) (col26 / scatter) or al16(mx_lds_bytes(B)) + kMxSparseBytes (MX), 52 B (scatter).
template <int BS, bool MX>
__device__ void run_task(const mul_large_args& g, const large_desc& d, uint32_t la, uint32_t lb, uint8_t* plds,
                         bool col26_ok = true) {
    uint32_t* S = g.scratch;
    const uint32_t LA = d.LA, LB = d.LB, Bm = g.Bm, nB = d.nB;
    const layer_src srcA = side_layer(&g.A, g.A.e_off[d.pair], S, d.o_lstA, LA, la);
    const layer_src srcB = side_layer(&g.B, g.B.e_off[d.pair], S, d.o_lstB, LB, lb);
    const uint32_t na = srcA.n, nb = srcB.n;
    const uint32_t lp = la * LB + lb;
    const uint64_t slot0 = (uint64_t)lp * Bm;
    const int tid = threadIdx.x;
    const bool denseA = na >= nb;
    const uint32_t nd = denseA ? na : nb, ns = denseA ? nb : na;
    const layer_src& Dn = denseA ? srcA : srcB;
    const layer_src& Sp = denseA ? srcB : srcA;
    const uint32_t tmulD = denseA ? nB : 1u, tmulS = denseA ? 1u : nB;   // shares of t = i |B.E| + j
    uint32_t* tkey = S + d.o_tkey;
    uint32_t* info = S + d.o_info;
    ulonglong2* sums = (ulonglong2*)(S + d.o_sums);
    // keys alone in their bucket are their own bucket leaders: mark them here, where the atomic
    // overlaps the multiply-bound loop of other waves, and `rank` skips them
    const uint32_t* ghead = group_heads(g, d);
    // iblk pairs: no block marks here (k_large_products_la counts per A edge; a pair that falls back
    // has its lone leaders marked by k_large_rank)
    unsigned long long* bpack = d.iblk ? nullptr : (unsigned long long*)w64(S, d.o_bmask);
    bool any = false;

    bool dense = col26_ok && nd >= kLargeDenseMin;
    if (MX && dense && ns <= kMxMaxSparse) {
        uint4* prec = (uint4*)(plds + mx_lds_bytes(Bm));
        uint4* pinf = prec + 3u * kMxMaxSparse;
        mx_stage_sparse(prec, pinf, Bm, Sp, tmulS, (uint32_t)tid);   // made visible by the dense staging's barriers
        dense = mx_stage_dense<BS>(plds, Bm, Dn, tmulD);
        if (dense) any = mx_blocks<BS>(plds, prec, pinf, ns, Bm, slot0, task_out{tkey, info, sums, ghead, bpack});
        __syncthreads();
    } else if (dense) {
        // Dense-owner mode with column accumulators (fp127.hpp col26_*): both sides are staged as
        // 26-bit limbs, each probe is 25 v_mad_u64_u32 into the lane's P or M columns and a
        // saturating add + min for the first-insert time. Empty dense slots hold zero limbs and
        // time kInf, so the loop has no branch: a miss adds 0 and leaves the time alone.
        uint4* dl4 = (uint4*)plds;
        uint2* dx = (uint2*)(plds + 64u * Bm);
        uint4* sl4 = (uint4*)(plds + al16(kDenseFixed * Bm));
        uint32_t* sl1 = (uint32_t*)(sl4 + kChunk);
        uint32_t* sinf = sl1 + kChunk;
        uint32_t* sidv = sinf + kChunk;
        uint32_t* dup = sidv + kChunk;
        // the first sparse chunk's loads go out before the dense staging, so the two sides' global
        // round trips overlap (thread k < kChunk < BS stages sparse edge k)
        edge_rec pr0{0, 0, 0, 0};
        if ((uint32_t)tid < min(ns, kChunk)) pr0 = load_edge(Sp, tid);
        for (uint32_t k = tid; k < 4 * Bm; k += BS) {
            dl4[k] = make_uint4(0, 0, 0, 0);
            dx[k] = make_uint2(0, kInf);
        }
        if (tid == 0) *dup = 0;
        __syncthreads();
        for (uint32_t k0 = tid; k0 < nd; k0 += 2u * BS) {   // two edges per round, loads first
            edge_rec x[2];
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const uint32_t k = k0 + (uint32_t)v * BS;
                x[v] = load_edge(Dn, k < nd ? k : 0u);
            }
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                if (k0 + (uint32_t)v * BS >= nd) break;
                const uint32_t sl = meta_ch(x[v].meta) * 2u * Bm + meta_idx(x[v].meta);
                // dx.y holds the dense side's share of the first-insert time t = i |B.E| + j
                const uint32_t te = x[v].e * tmulD;
                if (atomicCAS(&dx[sl].y, kInf, te) != kInf) {
                    *dup = 1;
                } else {   // canonical operands: the limb split needs a, b < 2^127
                    uint32_t l[5];
                    fp_split26(fp_canon(x[v].lo, x[v].hi), l);
                    dl4[sl] = dl4[sl + Bm] = make_uint4(l[0], l[1], l[2], l[3]);
                    dx[sl].x = l[4];
                    dx[sl + Bm] = make_uint2(l[4], te);
                }
            }
        }
        __syncthreads();
        dense = *dup == 0;   // duplicate (layer, idx, ch) edges: use the scatter mode instead
        if (dense) {
            const uint32_t rows = (Bm + BS - 1) / BS;   // workgroup-uniform (1 for B <= BS)
            for (uint32_t u = 0; u < rows; ++u) {
                const uint32_t r = tid + u * BS;
                const bool live = r < Bm;
                const uint4* dl4r = dl4 + (live ? r : 0u);
                const uint2* dxr = dx + (live ? r : 0u);
                uint64_t P[9], M[9];
                col26_zero(P);
                col26_zero(M);
                uint32_t tmin = kInf;
                for (uint32_t c0 = 0; c0 < ns; c0 += kChunk) {
                    const uint32_t cn = min(kChunk, ns - c0);
                    __syncthreads();
                    if ((uint32_t)tid < cn) {
                        const uint32_t k = (uint32_t)tid;
                        const bool first = u == 0 && c0 == 0;   // prefetched above
                        const edge_rec x = first ? pr0 : load_edge(Sp, c0 + k);
                        uint32_t l[5];
                        fp_split26(fp_canon(x.lo, x.hi), l);
                        sl4[k] = make_uint4(l[0], l[1], l[2], l[3]);
                        sl1[k] = l[4];
                        // wave-uniform offsets of the P and M slots relative to lane r: the dense
                        // channel equal to the sparse one gives P, the other M
                        const uint32_t sidx = meta_idx(x.meta), sch = meta_ch(x.meta);
                        sinf[k] = (sch * 2u * Bm + Bm - sidx) | (((sch ^ 1u) * 2u * Bm + Bm - sidx) << 16);
                        sidv[k] = x.e * tmulS;   // the sparse side's share of t
                    }
                    __syncthreads();
                    if (live) {
                        for (uint32_t q = 0; q < cn; ++q) {
                            const uint32_t so = __builtin_amdgcn_readfirstlane(sinf[q]);
                            const uint32_t oP = so & 0xFFFFu, oM = so >> 16;
                            const uint4 b4 = sl4[q];
                            const uint32_t b[5] = {b4.x, b4.y, b4.z, b4.w, sl1[q]};
                            const uint32_t se = sidv[q];
                            const uint4 p4 = dl4r[oP], m4 = dl4r[oM];
                            const uint2 px = dxr[oP], mx = dxr[oM];
                            const uint32_t ap[5] = {p4.x, p4.y, p4.z, p4.w, px.x};
                            const uint32_t am[5] = {m4.x, m4.y, m4.z, m4.w, mx.x};
                            col26_mac(P, ap, b);
                            col26_mac(M, am, b);
                            tmin = min(tmin, min(__builtin_elementwise_add_sat(px.y, se),
                                                 __builtin_elementwise_add_sat(mx.y, se)));
                        }
                        col26_norm(P);
                        col26_norm(M);
                    }
                }
                if (live) {
                    const uint64_t s = slot0 + r;
                    tkey[s] = tmin;
                    if (tmin != kInf) {
                        const fp ps = col26_fold(P), ms = col26_fold(M);
                        const uint32_t eb = (fp_nonzero(ps) ? 1u : 0u) | (fp_nonzero(ms) ? 2u : 0u);
                        info[s] = eb;
                        sums[2 * s] = make_ulonglong2(ps.lo, ps.hi);
                        sums[2 * s + 1] = make_ulonglong2(ms.lo, ms.hi);
                        any |= eb != 0;
                        if (eb && bpack && ghead && ghead[s] == 0u) leader_mark(bpack, tmin, __popc(eb));
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!dense) {
        unsigned long long* acc = (unsigned long long*)plds;
        uint32_t* tk = (uint32_t*)(plds + 48u * Bm);
        for (uint32_t k = tid; k < 6 * Bm; k += BS) acc[k] = 0ull;
        for (uint32_t k = tid; k < Bm; k += BS) tk[k] = kInf;
        __syncthreads();
        const uint64_t np = (uint64_t)na * nb;
        for (uint64_t t = tid; t < np; t += BS) {
            const uint32_t ai = (uint32_t)(t / nb), bj = (uint32_t)(t - (uint64_t)ai * nb);
            const edge_rec xa = load_edge(srcA, ai), xb = load_edge(srcB, bj);
            const uint32_t r = mod_small(meta_idx(xa.meta) + meta_idx(xb.meta), Bm);
            const uint32_t chn = meta_ch(xa.meta) ^ meta_ch(xb.meta);
            const fp pv = fp_mul(fp{xa.lo, xa.hi}, fp{xb.lo, xb.hi});
            uint64_t l0, l1, l2;
            fp_split3(pv, l0, l1, l2);
            unsigned long long* q = acc + (size_t)(r * 2 + chn) * 3;
            atomicAdd(q + 0, (unsigned long long)l0);
            atomicAdd(q + 1, (unsigned long long)l1);
            atomicAdd(q + 2, (unsigned long long)l2);
            atomicMin(&tk[r], xa.e * nB + xb.e);
        }
        __syncthreads();
        for (uint32_t r = tid; r < Bm; r += BS) {
            const uint64_t s = slot0 + r;
            const uint32_t tkr = tk[r];
            tkey[s] = tkr;
            if (tkr != kInf) {
                const unsigned long long* q = acc + (size_t)r * 6;
                const fp p = fp_fold3(q[0], q[1], q[2]);
                const fp m = fp_fold3(q[3], q[4], q[5]);
                const uint32_t eb = (fp_nonzero(p) ? 1u : 0u) | (fp_nonzero(m) ? 2u : 0u);
                info[s] = eb;
                sums[2 * s] = make_ulonglong2(p.lo, p.hi);
                sums[2 * s + 1] = make_ulonglong2(m.lo, m.hi);
                any |= eb != 0;
                if (eb && bpack && ghead && ghead[s] == 0u) leader_mark(bpack, tkr, __popc(eb));
            }
        }
        __syncthreads();   // the caller may reuse the LDS
    }
    if (any) S[d.o_used + (LA + LB) + lp] = 1;   // benign race: every writer stores 1
}

// one workgroup per task (la, lb): pairs with many B layers (squares)
template <int BS>
__global__ __launch_bounds__(BS) void k_large_products(mul_large_args g) {
    extern __shared__ __attribute__((aligned(16))) uint8_t plds[];
    const large_desc& d = g.desc[g.sel[g.n_la + blockIdx.y]];
    uint32_t* S = g.scratch;
    const uint32_t* cnt = S + d.o_cnt;
    if (cnt[kCntInvalid]) return;
    const uint32_t LB = d.LB;
    const uint32_t tl = blockIdx.x;
    const uint32_t la_i = tl / LB, lb_i = tl - la_i * LB;
    if (la_i >= cnt[kCntNeA] || lb_i >= cnt[kCntNeB]) return;
    run_task<BS, true>(g, d, S[d.o_neA + la_i], S[d.o_neB + lb_i], plds);
}

// ---- per-A-edge emit order (iblk pairs) ---------------------------------------------------
// The reference emits keys in hash-list order: bucket first-insert time DESC, then key time DESC
// (see k_mul_fresh.hip). A first-insert time t = i |B.E| + j names A edge i and B edge j, and the
// key lies in product layer (layer(i), layer(j)): every key whose time falls in A edge i's range
// [i |B.E|, (i + 1) |B.E|) belongs to ONE A layer, which one k_large_products_la workgroup
// multiplies against every B layer. So that workgroup can count the edges of A edge i's keys and
// rank each key among them (by j DESC) in LDS; a suffix scan over the |A.E| counts then gives
// every key's position: offset(i) + rank. This replaces the n/16-word block marks (zeroed, marked
// with random 64-bit atomics, scanned and read back at random: k_large_init / products / scan /
// order) with |A.E| plain counts. Keys that share a libstdc++ bucket with another slot of the
// static group (a few percent) are emitted at their bucket leader's time: k_large_rank moves their
// edges from their own A edge's count to the leader's, and every A edge range holding such a key
// is flagged so that `order` ranks its keys by probing the range's |B.E| times instead.

// After the tasks of A layer la (all B layers) have left one record per key in recs (the MFMA
// epilogue: the dense slot d of the key's A edge, its B edge j, its edge bits): M1[d] / M2[d] = bit j
// for the keys whose first-insert time is (A edge at d, B edge j) and that emit a P / an M edge,
// bit 63 of M1 = a key of a shared bucket lies in the range (`order` probes it); then icnt[i] and,
// for ranges with keys, imask[i] = (M1, M2). M1 / M2 use the dense digit table's LDS (dead now), tt
// maps dense slot d back to its A edge. Barriers inside; every thread calls it.
template <int BS>
__device__ void iblk_layer(uint8_t* plds, const mul_large_args& g, const large_desc& d, uint32_t neB, const uint32_t* recs,
                           uint32_t* icnt, ulonglong2* imask) {
    const uint32_t Bm = g.Bm, nB = d.nB;
    uint32_t* S = g.scratch;
    unsigned long long* M1 = (unsigned long long*)plds;
    unsigned long long* M2 = M1 + 2u * Bm;
    const uint32_t* tt = (const uint32_t*)(plds + mx_tt_off(Bm));
    const uint64_t m = d.nb_m;
    const uint32_t tid = threadIdx.x, nk = neB * Bm;
    for (uint32_t k = tid; k < 4u * Bm; k += BS) M1[k] = 0ull;
    __syncthreads();
    bool shared = false;
    for (uint32_t q = tid; q < nk; q += BS) {
        const uint32_t v = recs[q];
        if (!v) continue;
        const uint32_t dd = v & 0xFFFu, j = (v >> 12) & 63u, e = (v >> 18) & 3u;
        if (e & 1u) atomicOr(&M1[dd], 1ull << j);
        if (e & 2u) atomicOr(&M2[dd], 1ull << j);
        if (v & kRecShared) {   // with or without edges: it may lead its bucket
            atomicOr(&M1[dd], 1ull << 63);
            shared = true;
        }
    }
    if (shared) S[d.o_cnt + kCntIShared] = 1u;
    __syncthreads();
    for (uint32_t dd = tid; dd < 2u * Bm; dd += BS) {
        const uint32_t ch = dd >= Bm ? 1u : 0u;
        const uint32_t te = tt[dd + ch * Bm];   // tt slot ch 2B + idx
        if (te == kInf) continue;
        uint32_t j;
        const uint32_t i = div_small(te, nB, m, j);
        const unsigned long long x1 = M1[dd], x2 = M2[dd];
        icnt[i] = (uint32_t)__popcll(x1 & ~(1ull << 63)) + (uint32_t)__popcll(x2);
        // only ranges that hold keys are read back (write_ranges, order): most A edges of a deep
        // chain step hold none (their keys were all inserted by earlier A edges)
        if (x1 | x2) imask[i] = make_ulonglong2(x1, x2);
    }
    __syncthreads();   // the next A layer's staging overwrites M1 / M2, tt and recs
}

// One workgroup per (pair, kLaPerWG A layers) for pairs with at most kLaMaxLB B layers (chain
// steps): the B layers' sparse sides are staged once per workgroup and each A layer's dense table
// once for all B layers, so a chain step reads every A edge once (a task per workgroup read it
// |B.L| times) and pays the dependent header loads once per kLaPerWG x |B.L| tasks. The kernel is
// latency-bound: 4 workgroups per CU (<= 128 VGPRs, 32 KB of LDS) against 3: -10%; forced to 96
// VGPRs for 5 per CU it was 28% slower.
// Tasks the matrix-core mode does not take: sparse x sparse (and layers with duplicate edges) run
// the scatter mode in place; dense tasks with a large sparse side (column mode, 33 KB of LDS) go to
// a per-pair list for k_large_products_defer.
template <int BS>
__global__ __launch_bounds__(BS, kLaMinBlocks) void k_large_products_la(mul_large_args g) {
    extern __shared__ __attribute__((aligned(16))) uint8_t plds[];
    uint32_t py = blockIdx.y, px = blockIdx.x;
    if (g.la_xcd) {   // workgroups go to XCDs round-robin by linear id: XCD x takes pairs x, x + 8, ...
        const uint32_t lin = blockIdx.x + blockIdx.y * gridDim.x, k = lin >> 3;
        py = (k / gridDim.x) * 8u + (lin & 7u);
        px = k % gridDim.x;
        if (py >= g.n_la) return;
    }
    const large_desc& d = g.desc[g.sel[py]];
    if (d.direct) return;   // k_large_products_direct
    uint32_t* S = g.scratch;
    const uint32_t* cnt = S + d.o_cnt;
    if (cnt[kCntInvalid]) return;
    const uint32_t neA = cnt[kCntNeA], neB = min(cnt[kCntNeB], kLaMaxLB);   // the host sends pairs with |B.L| <= kLaMaxLB
    const uint32_t i0 = px * g.la_per_wg;
    if (i0 >= neA) return;
    const uint32_t LA = d.LA, LB = d.LB, Bm = g.Bm, nB = d.nB;
    uint8_t* sreg = plds + g.lds_task;   // per B layer: prec | pinf
    uint32_t lbv[kLaMaxLB], nbv[kLaMaxLB];
    uint32_t okm = 0;   // B layers staged as MX sparse sides
#pragma unroll
    for (uint32_t k = 0; k < kLaMaxLB; ++k) {
        lbv[k] = 0;
        nbv[k] = 0;
        if (k < neB) {
            const uint32_t lb = S[d.o_neB + k];
            const layer_src srcB = side_layer(&g.B, g.B.e_off[d.pair], S, d.o_lstB, LB, lb);
            lbv[k] = lb;
            nbv[k] = srcB.n;
            if (srcB.n <= kMxMaxSparse) {
                okm |= 1u << k;
                uint4* prec = (uint4*)(sreg + k * kMxSparseBytes);
                mx_stage_sparse(prec, prec + 3u * kMxMaxSparse, Bm, srcB, 1u, threadIdx.x);
            }
        }
    }
    // iblk: per-A-edge counts and ranks (iblk_layer) instead of block marks, unless the pair has
    // fallen back (cnt[kCntIFail], set by k_large_lists or by a workgroup below)
    bool ib = d.iblk && !S[d.o_cnt + kCntIFail];
    uint32_t* bjt = (uint32_t*)(sreg + kLaMaxLB * kMxSparseBytes);   // B edge j: idx | ch << 16
    uint32_t* recs = bjt + 64;                                           // [kLaMaxLB][B] key records
    if (ib && threadIdx.x < nB) {   // published by the dense staging's barriers
        const uint64_t mb = g.B.meta[g.B.e_off[d.pair] + threadIdx.x];
        bjt[threadIdx.x] = meta_idx(mb) | meta_ch(mb) << 16;
    }
    const task_out o{S + d.o_tkey, S + d.o_info, (ulonglong2*)(S + d.o_sums), group_heads(g, d),
                     d.iblk ? nullptr : (unsigned long long*)w64(S, d.o_bmask)};
    const uint32_t i1 = min(neA, i0 + g.la_per_wg);
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t la = S[d.o_neA + i];
        const layer_src srcA = side_layer(&g.A, g.A.e_off[d.pair], S, d.o_lstA, LA, la);
        const uint32_t na = srcA.n;
        uint32_t mxm = 0;   // B layers whose task with this A layer runs on the matrix cores
        bool dupA = false;
        if (na >= kLargeDenseMin)
#pragma unroll
            for (uint32_t k = 0; k < kLaMaxLB; ++k)
                if (((okm >> k) & 1u) && na >= nbv[k]) mxm |= 1u << k;
        if (mxm) {
            if (mx_stage_dense<BS>(plds, Bm, srcA, nB)) {   // barriers inside (they also publish the B staging)
#pragma unroll
                for (uint32_t k = 0; k < kLaMaxLB; ++k) {
                    if (!((mxm >> k) & 1u)) continue;
                    const uint4* prec = (const uint4*)(sreg + k * kMxSparseBytes);
                    const uint32_t lp = la * LB + lbv[k];
                    task_out ok = o;
                    if (ib) {
                        ok.recs = recs + k * Bm;
                        ok.bjt = bjt;
                        ok.nB = nB;
                        ok.nb_m = d.nb_m;
                    }
                    if (mx_blocks<BS>(plds, prec, prec + 3u * kMxMaxSparse, nbv[k], Bm, (uint64_t)lp * Bm, ok))
                        S[d.o_used + (LA + LB) + lp] = 1;
                }
            } else {
                mxm = 0;   // duplicate edges in this A layer: its tasks take run_task's scatter mode
                dupA = true;
            }
            __syncthreads();
        }
        for (uint32_t k = 0; k < neB; ++k) {
            if ((mxm >> k) & 1u) continue;
            if (!dupA && max(na, nbv[k]) >= kLargeDenseMin) {
                if (threadIdx.x == 0) S[d.o_defer + atomicAdd((uint32_t*)cnt + kCntDefer, 1u)] = i << 16 | k;
            } else {
                run_task<BS, false>(g, d, la, lbv[k], plds, false);   // scatter mode
            }
        }
        if (ib) {
            // every task of this A layer ran on the matrix cores (its dense table staged, no duplicate
            // (idx, ch) edges): count and rank per A edge; otherwise the pair falls back
            if (mxm == (1u << neB) - 1u) {
                iblk_layer<BS>(plds, g, d, neB, recs, S + d.o_icnt, (ulonglong2*)(S + d.o_imask));
            } else {
                if (threadIdx.x == 0) atomicExch(&S[d.o_cnt + kCntIFail], 1u);
                ib = false;
            }
        }
    }
}

// the column-mode tasks k_large_products_la deferred: kDeferWG workgroups per pair walk its list
constexpr uint32_t kDeferWG = 4;
template <int BS>
__global__ __launch_bounds__(BS) void k_large_products_defer(mul_large_args g) {
    extern __shared__ __attribute__((aligned(16))) uint8_t plds[];
    const large_desc& d = g.desc[g.sel[blockIdx.y]];
    if (d.direct) return;
    uint32_t* S = g.scratch;
    const uint32_t* cnt = S + d.o_cnt;
    if (cnt[kCntInvalid]) return;
    const uint32_t nq = cnt[kCntDefer];
    for (uint32_t q = blockIdx.x; q < nq; q += kDeferWG) {
        const uint32_t v = S[d.o_defer + q];
        run_task<BS, false>(g, d, S[d.o_neA + (v >> 16)], S[d.o_neB + (v & 0xFFFFu)], plds);
    }
}

}  // namespace

// products: the matrix-core dense mode in 4-wave workgroups (A-layer-major for pairs with few B
// layers, one task per workgroup for the rest)
void launch_large_products(const mul_large_args& a, hipStream_t st) {
    const unsigned nl = a.nl;
    const size_t plds = prod_lds_bytes(a.Bm);
    const size_t lx = std::max<size_t>(plds, mx_lds_bytes(a.Bm) + kMxSparseBytes);
    if (nl > a.n_la && a.max_tasks)
        hipLaunchKernelGGL((k_large_products<kLPX>), dim3((unsigned)a.max_tasks, nl - a.n_la), dim3(kLPX), lx, st, a);
    if (a.n_la && a.max_la_wg) {
        mul_large_args b = a;
        b.lds_task = mx_lds_bytes(a.Bm);   // the scatter mode (52 B per slot) fits below it
        hipLaunchKernelGGL((k_large_products_la<kLPX>), dim3((unsigned)a.max_la_wg, a.la_xcd ? (a.n_la + 7u) & ~7u : a.n_la),
                           dim3(kLPX), (size_t)b.lds_task + kLaMaxLB * kMxSparseBytes + kIblkBjtBytes + kLaMaxLB * 4u * a.Bm,
                           st, b);
        hipLaunchKernelGGL((k_large_products_defer<kLPX>), dim3(kDeferWG, a.n_la), dim3(kLPX), plds, st, a);
    }
}

}  // namespace pvhip
