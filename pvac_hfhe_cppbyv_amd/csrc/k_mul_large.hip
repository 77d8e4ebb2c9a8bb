// k_mul_large.hip — batched ct_mul for general pairs (reference ops/arithmetic.hpp:47-106):
// chains c_k = c_{k-1} * x (test_main.cpp:289-295), squares (test_depth.cpp:46), any pair the
// LDS-resident fresh kernel cannot hold.
//
// The reference aggregates |A.E||B.E| products in one std::unordered_map. Here the product
// space is cut along its natural independence: every product of an A edge in layer la and a
// B edge in layer lb lands in product layer lp = la*LB + lb, a cyclic convolution of length B
// over Fp with +/- channels. One workgroup owns one (la, lb) TASK:
//   dense-owner mode : the side with more edges becomes a dense [2][B] table of 26-bit limbs in
//                      LDS; one lane per output index r loops over the other side's edges and
//                      accumulates P/M sums as nine u64 columns each (25 v_mad_u64_u32 per
//                      product, no carry chain; fp127.hpp col26_*) and the key's first-insert time
//                      in REGISTERS (no atomics). For saturated chain layers (674 edges) every
//                      probe is useful.
//   scatter mode     : sparse x sparse tasks (and inputs with duplicate (layer, idx, ch) edges)
//                      accumulate 43/42/42-bit limbs with LDS atomics, as the fresh kernel.
// Results go to a dense per-pair key-slot array [|A.L||B.L|][B] in global scratch.
//
// The reference's emit order (hash-table list order: bucket first-insert time DESC, key
// first-insert time DESC; see k_mul_fresh.hip) is rebuilt without sorting:
//   link  : key -> libstdc++ bucket (hash * 0x9E37... mod bucket_count), bucket chains through
//           a global open-addressing table keyed by bucket id;
//   rank  : each key walks its (short) chain: bucket first-insert time t_b, edges of its bucket
//           emitted before it; bucket leaders mark bit t_b in a 64-bit mask per 64 first-insert
//           times and add their bucket's edge count to that block;
//   scan  : suffix scan over blocks (n/64 entries, not n);
//   order : position = block offset + edges of leaders later in the same block (mask bits above,
//           each resolved to its key slot from the leader's (i, j) = (t / |B.E|, t % |B.E|)) +
//           rank inside the bucket; slot ids are scattered into an order array (4 B each);
//   write : one coalesced pass writes (meta, w) in order.
// compact_layers (encrypt.hpp:73-104) runs per pair between aggregation and write, so edges
// are written once with their final layer ids; guard_budget (encrypt.hpp:106-111) switches a
// pair to (layer, idx, P<M) order when its edge count exceeds edge_budget.
//
// The stages in launch order (launch_ct_mul_large, at the end of this file) and their files:
//   init, lists                                   here
//   direct pairs: count_la, scan_direct           k_large_direct.hip
//                 layers (their pass)             here
//                 products_direct, direct_redo    k_large_direct.hip
//   products, products_la, products_defer         k_large_products.hip
//   layers, link, rank, scan, order, write,       here
//   write_ranges
// A deep pair (more than kLargeLayersMax layers before compaction: the LDS tables of lists and layers)
// runs its own lists and layers kernels between these stages (k_large_deep.hip, launch_ct_mul_large_deep).
// Outside the sequence: static bucket groups, chain images -> records (k_large_aux.hip). Shared
// device pieces: k_large.hpp; the matrix-core pieces of the products kernels: k_large_mx.hpp.
#include "compact_layers.hpp"
#include "k_large.hpp"

namespace pvhip {

namespace {

// ---------------------------------------------------------------- init
// iblk pairs leave the block marks alone (k_large_layers clears them for a pair that falls back)
// and tkey (iblk_dead): only cnt and the used flags are zeroed (static groups have no bucket table)
__global__ __launch_bounds__(kLB) void k_large_init(mul_large_args g) {
    const large_desc& d = g.desc[blockIdx.y];
    const uint64_t stride = (uint64_t)gridDim.x * kLB;
    const uint64_t nz = d.iblk ? kCntWords + d.Lc : d.zero_words;
    const uint64_t nt = d.iblk ? 0 : d.S;   // iblk: products sets every slot of a live layer pair
    const uint64_t lim = nz > nt ? nz : nt;
    for (uint64_t w = (uint64_t)blockIdx.x * kLB + threadIdx.x; w < lim; w += stride) {
        if (w < nz) g.scratch[d.iblk && w >= kCntWords ? d.o_used + (w - kCntWords) : d.o_zero + w] = 0;
        if (w < nt) g.scratch[d.o_tkey + w] = kInf;
    }
}

// ---------------------------------------------------------------- per-layer edge lists
// One workgroup per pair: validates edges (layer < |L|, idx < B, ch <= 1), buckets edge ids
// by layer (any order inside a layer: first-insert times are minima, not positions) and
// lists the non-empty layers of both sides.
constexpr uint32_t kListRegRounds = 8;   // rounds of 4 x kLBig A edges whose pass 2 reads registers
static_assert(kLargeLayersMax <= (1u << 15), "k_large_lists packs a layer in 15 bits");
__global__ __launch_bounds__(kLBig) void k_large_lists(mul_large_args g) {
    extern __shared__ __attribute__((aligned(16))) uint32_t hist[];   // [LA + LB] counts, then cursors
    __shared__ uint32_t flag;
    const large_desc& d = g.desc[blockIdx.x];
    const uint64_t pr = d.pair;
    const uint32_t LA = d.LA, LB = d.LB, nA = d.nA, nB = d.nB, Bm = g.Bm;
    const uint64_t aeo = g.A.e_off[pr], beo = g.B.e_off[pr];
    uint32_t* S = g.scratch;
    uint32_t* cnt = S + d.o_cnt;
    const int tid = threadIdx.x;
    for (uint32_t l = tid; l < LA + LB; l += kLBig) hist[l] = 0;
    if (tid == 0) flag = 0;
    __syncthreads();
    // A as a dense chain image (mul_large_args::A_img, written by the previous step's
    // k_large_products_direct): layer l >= first holds the 2B edges [(l - first) 2B, (l - first + 1) 2B)
    // in cell order, and 32-bit word s of the pair's meta region is slot s's direct id (hash-order
    // edge | cell << 21): the lists are the slabs themselves, nothing to validate or bucket
    const bool aimg = g.A_img && g.A_img[pr];
    const uint32_t slab = 2u * Bm;
    const uint32_t nslab = aimg ? nA / slab : 0u;
    const uint32_t first = aimg && nslab <= LA ? LA - nslab : 0u;
    if (aimg) {
        for (uint32_t l = first + tid; l < LA; l += kLBig) hist[l] = slab;
        if (tid == 0 && (nslab > LA || nslab * slab != nA || !d.direct)) flag = 1;
    }
    // four edges per thread and round, loads first; the first kListRegRounds rounds keep each edge's
    // layer and cell in registers for the scatter pass (layer < 2^15, cell < 2^11), later rounds
    // load their metas again
    uint32_t pk[kListRegRounds][4];
    auto hist_round = [&](uint32_t i0, uint32_t (&pr)[4]) {
        uint64_t m[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = i0 + (uint32_t)u * kLBig;
            m[u] = i < nA ? g.A.meta[aeo + i] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            pr[u] = meta_layer(m[u]) | (meta_ch(m[u]) * Bm + meta_idx(m[u])) << 15;
            if (i0 + (uint32_t)u * kLBig >= nA) continue;
            const uint32_t la = meta_layer(m[u]);
            if (la >= LA || meta_idx(m[u]) >= Bm || meta_ch(m[u]) > 1) flag = 1;
            else atomicAdd(&hist[la], 1u);
        }
    };
    if (!aimg) {
#pragma unroll
        for (uint32_t r = 0; r < kListRegRounds; ++r)
            if (tid + r * 4u * kLBig < nA) hist_round(tid + r * 4u * kLBig, pk[r]);
        for (uint32_t i0 = tid + kListRegRounds * 4u * kLBig; i0 < nA; i0 += 4u * kLBig) {
            uint32_t pr[4];
            hist_round(i0, pr);
        }
    }
    for (uint32_t j = tid; j < nB; j += kLBig) {
        const uint64_t m = g.B.meta[beo + j];
        const uint32_t lb = meta_layer(m);
        if (lb >= LB || meta_idx(m) >= Bm || meta_ch(m) > 1) flag = 1;
        else atomicAdd(&hist[LA + lb], 1u);
    }
    __syncthreads();
    if (flag) {   // invalid references: reject the pair (reference behaviour is UB)
        if (tid == 0) {
            cnt[kCntInvalid] = 1;
            g.pair_status[pr] = 2;
            g.C.l_cnt[pr] = 0;
            g.C.e_cnt[pr] = 0;
        }
        return;
    }
    // layer ranges by atomic allocation; non-empty layer lists by atomic append
    for (uint32_t l = tid; l < LA + LB; l += kLBig) {
        const uint32_t c = hist[l];
        if (d.iblk && l >= LA && c > kIblkMaxSparse) cnt[kCntIFail] = 1;   // its tasks would be deferred
        const bool a = l < LA;
        uint32_t* lst = a ? S + d.o_lstA : S + d.o_lstB;
        const uint32_t ll = a ? l : l - LA;
        const uint32_t L = a ? LA : LB;
        uint32_t start = 0;
        if (c) {
            start = atomicAdd(&cnt[a ? kCntAllocA : kCntAllocB], c);
            if (aimg && a) start = (ll - first) * slab;   // the layer's slab
            const uint32_t k = atomicAdd(&cnt[a ? kCntNeA : kCntNeB], 1u);
            (S + (a ? d.o_neA : d.o_neB))[k] = ll;
        }
        lst[ll] = start;
        lst[L + ll] = c;
        hist[l] = start;   // cursor
    }
    __syncthreads();
    uint32_t* idsA = S + d.o_lstA + 2 * LA;
    uint32_t* idsB = S + d.o_lstB + 2 * LB;
    if (d.direct) {   // k_large_count_la stores the count bytes of the A edges whose ranges hold keys only
        uint4* z = (uint4*)(S + d.o_icnt);
        for (uint32_t i = tid; i < 2u * ((nA + 31u) >> 5); i += kLBig) z[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    // direct pairs: an A id carries its dense cell, i | (ch B + idx) << 21 (the host checked
    // |A.E| < 2^21, B <= 1024), so their passes need no per-edge meta gather
    const uint32_t dsh = d.direct ? 21u : 32u;
    auto scatter_round = [&](uint32_t i0, const uint32_t (&pr)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = i0 + (uint32_t)u * kLBig;
            if (i >= nA) break;
            const uint64_t cell = pr[u] >> 15;
            idsA[atomicAdd(&hist[pr[u] & 0x7FFFu], 1u)] = i | (uint32_t)((cell << dsh) & 0xFFFFFFFFull);
        }
    };
    if (!aimg) {   // (an image's ids sit in its meta region: the direct kernels read them there)
#pragma unroll
        for (uint32_t r = 0; r < kListRegRounds; ++r)
            if (tid + r * 4u * kLBig < nA) scatter_round(tid + r * 4u * kLBig, pk[r]);
    }
    for (uint32_t i0 = tid + kListRegRounds * 4u * kLBig; i0 < nA && !aimg; i0 += 4u * kLBig) {
        uint64_t m[4];
        uint32_t pr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = i0 + (uint32_t)u * kLBig;
            m[u] = i < nA ? g.A.meta[aeo + i] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) pr[u] = meta_layer(m[u]) | (meta_ch(m[u]) * Bm + meta_idx(m[u])) << 15;
        scatter_round(i0, pr);
    }
    for (uint32_t j = tid; j < nB; j += kLBig) {
        const uint32_t lb = meta_layer(g.B.meta[beo + j]);
        idsB[atomicAdd(&hist[LA + lb], 1u)] = j;
    }
}

// ---------------------------------------------------------------- compact_layers + layer records
// One workgroup per pair (encrypt.hpp:73-104): keep = product layers with emitted edges, plus
// transitive PROD parents; remap by exclusive count; write the kept records (product-layer
// ztags computed here, only for kept layers) and leave the remap in scratch for the writer.
__global__ __launch_bounds__(kLBig) void k_large_layers(mul_large_args g) {
    extern __shared__ __attribute__((aligned(16))) uint32_t keep[];   // [Lc]
    __shared__ uint32_t changed;
    __shared__ uint32_t part[kLBig / 64];
    const large_desc& d = g.desc[blockIdx.x];
    uint32_t* S = g.scratch;
    if (S[d.o_cnt + kCntInvalid]) return;
    // direct pairs: their own pass before their products (redone pairs: none); the others after
    if (g.layers_direct ? !(d.direct && S[d.o_cnt + kCntDirect]) : d.direct != 0) return;
    const uint64_t pr = d.pair;
    const uint32_t LA = d.LA, LB = d.LB, Lc = (uint32_t)d.Lc, base = LA + LB;
    const uint64_t alo = g.A.l_off[pr], blo = g.B.l_off[pr], clo = g.C.l_off[pr];
    uint32_t* used = S + d.o_used;
    const int tid = threadIdx.x;
    if (d.iblk && S[d.o_cnt + kCntIFail])   // k_large_rank marks this pair's leaders next
        for (uint64_t w = tid; w < 2 * d.nblk; w += kLBig) S[d.o_bmask + w] = 0;
    for (uint32_t l = tid; l < Lc; l += kLBig) keep[l] = l >= base ? (used[l] != 0) : 0u;
    block_close<kLBig>(keep, Lc, &changed, [&](uint32_t l, uint32_t& rule, uint32_t& pa, uint32_t& pb) {
        layer_parents(g, alo, blo, LA, LB, l, rule, pa, pb);
    });
    const uint32_t kept = block_remap<kLBig>(keep, keep, Lc, part);
    const bool identity = kept == Lc;
    for (uint32_t l = tid; l < Lc; l += kLBig) {
        const uint32_t to = keep[l];
        used[l] = to;   // remap for the edge writer
        if (to == kDropped) continue;
        pvac_layer y = layer_record(g, alo, blo, clo, LA, LB, l);
        remap_parents(y, keep, Lc, identity);
        g.C.layers[clo + to] = y;
    }
    if (tid == 0) g.C.l_cnt[pr] = kept;
}

// ---------------------------------------------------------------- bucket chains
__global__ __launch_bounds__(kLB) void k_large_link(mul_large_args g) {
    const large_desc& d = g.desc[blockIdx.y];
    if (d.direct) return;
    uint32_t* S = g.scratch;
    if (S[d.o_cnt + kCntInvalid]) return;
    const uint32_t Bm = g.Bm;
    const uint32_t* tkey = S + d.o_tkey;
    uint32_t* info = S + d.o_info;
    uint32_t* nxt = S + d.o_nxt;
    unsigned long long* hkey = (unsigned long long*)w64(S, d.o_hkey);
    uint32_t* hhead = S + d.o_hhead;
    const uint64_t hmask = (1ull << d.hbits) - 1;
    if (d.g_head != kNoGrp) return;   // static bucket groups: no per-pair chains
    for (uint64_t s = (uint64_t)blockIdx.x * kLB + threadIdx.x; s < d.S; s += (uint64_t)gridDim.x * kLB) {
        if (tkey[s] == kInf) continue;
        const uint64_t lp = s / Bm, r = s - lp * Bm;
        const uint64_t key = (lp << 32) | r;
        const uint64_t b = fmod64(key * kGolden, d.nbm);          // std::hash -> bucket
        uint64_t h = ((b + 1) * kGolden) >> (64 - d.hbits);
        for (;;) {
            const unsigned long long prev = atomicCAS(&hkey[h], 0ull, (unsigned long long)(b + 1));
            if (prev == 0ull || prev == b + 1) break;
            h = (h + 1) & hmask;
        }
        nxt[s] = atomicExch(&hhead[h], (uint32_t)(s + 1));
        info[s] = (info[s] & 3u) | ((uint32_t)h << 2);
    }
}

__global__ __launch_bounds__(kLB) void k_large_rank(mul_large_args g) {
    const large_desc& d = g.desc[blockIdx.y];
    if (d.direct) return;
    uint32_t* S = g.scratch;
    if (S[d.o_cnt + kCntInvalid]) return;
    const uint32_t* tkey = S + d.o_tkey;
    const uint32_t* info = S + d.o_info;
    const uint32_t* nxt = S + d.o_nxt;
    const uint32_t* hhead = S + d.o_hhead;
    uint32_t* tb = S + d.o_tb;
    uint32_t* within = S + d.o_within;
    uint32_t* etot = S + d.o_etot;
    unsigned long long* bpack = (unsigned long long*)w64(S, d.o_bmask);
    const bool stat = d.g_head != kNoGrp;
    const uint32_t* ghead = g.grp + (stat ? d.g_head : 0);
    const uint32_t* gnext = g.grp + (stat ? d.g_next : 0);
    // iblk: bucket-sharing keys move their edges to their leader's A edge count; a pair that fell
    // back marks blocks here, lone leaders included (products did not)
    const bool fb = d.iblk && S[d.o_cnt + kCntIFail];
    const bool ib = d.iblk && !fb;
    if (ib && !S[d.o_cnt + kCntIShared]) return;   // every key alone in its bucket: nothing to rank
    uint32_t* icnt = S + d.o_icnt;
    const uint64_t m = d.nb_m;
    for (uint64_t s = (uint64_t)blockIdx.x * kLB + threadIdx.x; s < d.S; s += (uint64_t)gridDim.x * kLB) {
        // static groups: a key alone in its bucket (the common case) was counted by `products`
        // and `order` takes t_b = its own time, within = 0
        const uint32_t q0 = stat ? ghead[s] : 1u;
        if (!q0 && fb) {
            if (iblk_dead(S, d, s, g.Bm)) continue;
            const uint32_t t = tkey[s];
            const uint32_t E = t == kInf ? 0u : __popc(info[s] & 3u);
            if (E) leader_mark(bpack, t, E);
            continue;
        }
        if (!q0 || iblk_dead(S, d, s, g.Bm)) continue;
        const uint32_t t = tkey[s];
        if (t == kInf) continue;
        uint32_t tmin = t, w = 0, E = 0;
        if (stat) {
            // the bucket's slots are a static property of (bucket count, B): walk them, keep the
            // ones present in this pair
            uint32_t q = q0;
            while (q) {
                const uint32_t s2 = q - 1;
                q = gnext[s2];
                if (s2 >= d.S || iblk_dead(S, d, s2, g.Bm)) continue;
                const uint32_t t2 = tkey[s2];
                if (t2 == kInf) continue;
                const uint32_t e2 = __popc(info[s2] & 3u);
                tmin = t2 < tmin ? t2 : tmin;
                w += t2 > t ? e2 : 0u;
                E += e2;
            }
        } else {
            uint32_t q = hhead[info[s] >> 2];
            while (q) {
                const uint32_t s2 = q - 1;
                const uint32_t t2 = tkey[s2];
                const uint32_t e2 = __popc(info[s2] & 3u);
                tmin = t2 < tmin ? t2 : tmin;
                w += t2 > t ? e2 : 0u;
                E += e2;
                q = nxt[s2];
            }
        }
        tb[s] = tmin;
        within[s] = w;
        if (tmin == t) {
            etot[s] = E;
            if (E && !ib) leader_mark(bpack, t, E);   // one atomic per leader
        } else if (ib) {
            // products counted this key's edges in its own A edge's range: move them to the leader's
            const uint32_t e = __popc(info[s] & 3u);
            uint32_t j;
            const uint32_t is = div_small(t, d.nB, m, j), il = div_small(tmin, d.nB, m, j);
            if (e && is != il) {
                atomicSub(&icnt[is], e);
                atomicAdd(&icnt[il], e);
            }
        }
    }
}

// One workgroup per pair: suffix exclusive scan of the block counts (emit offsets), the
// total, the guard_budget decision and, for canonical pairs, canonical positions.
__global__ __launch_bounds__(kLBig) void k_large_scan(mul_large_args g) {
    __shared__ uint32_t part[kLBig / 64];
    const large_desc& d = g.desc[blockIdx.x];
    if (d.direct) return;   // k_large_scan_direct
    uint32_t* S = g.scratch;
    uint32_t* cnt = S + d.o_cnt;
    if (cnt[kCntInvalid]) return;
    const int tid = threadIdx.x;
    unsigned long long* bpack = (unsigned long long*)w64(S, d.o_bmask);
    const uint32_t nblk = (uint32_t)d.nblk;
    uint32_t total = 0;
    if (d.iblk && !cnt[kCntIFail]) {
        // per-A-edge counts -> exclusive suffix offsets in place (A edge nA-1 first), as below
        uint32_t* icnt = S + d.o_icnt;
        const uint32_t nA = d.nA;
        for (uint32_t base = 0; base < nA; base += 4u * kLBig) {
            const uint32_t r0 = base + 4u * (uint32_t)tid;
            uint32_t v[4];
            uint32_t local = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t r = r0 + (uint32_t)k;
                v[k] = r < nA ? icnt[nA - 1 - r] : 0u;
                local += v[k];
            }
            uint32_t tot;
            uint32_t run = total + block_exclusive_scan<kLBig>(local, part, tot);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t r = r0 + (uint32_t)k;
                if (r < nA) icnt[nA - 1 - r] = run;
                run += v[k];
            }
            total += tot;
        }
    }
    // reversed block index r (block nblk-1-r) in rounds of 4 kLBig: thread t takes r = base + 4t .. 4t+3
    // (adjacent threads, adjacent words: coalesced), one workgroup scan per round
    for (uint32_t base = 0; base < (d.iblk && !cnt[kCntIFail] ? 0u : nblk); base += 4u * kLBig) {
        const uint32_t r0 = base + 4u * (uint32_t)tid;
        unsigned long long v[4];
        uint32_t local = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t r = r0 + (uint32_t)k;
            v[k] = r < nblk ? bpack[nblk - 1 - r] : 0ull;
            local += (uint32_t)(v[k] >> 32);
        }
        uint32_t tot;
        uint32_t run = total + block_exclusive_scan<kLBig>(local, part, tot);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t r = r0 + (uint32_t)k;
            if (r < nblk) bpack[nblk - 1 - r] = ((unsigned long long)run << 32) | (v[k] & 0xFFFFFFFFull);
            run += (uint32_t)(v[k] >> 32);
        }
        total += tot;
    }
    const bool canonical = (g.flags & PVAC_MUL_ORDER_CANONICAL) != 0 || total > g.edge_budget;
    if (tid == 0) {
        cnt[kCntTotal] = total;
        cnt[kCntCanonical] = canonical;
        g.C.e_cnt[d.pair] = total;
        g.pair_status[d.pair] = canonical ? 1 : 0;
    }
    if (!canonical) return;
    const uint32_t* tkey = S + d.o_tkey;
    const uint32_t* info = S + d.o_info;
    uint32_t* cpos = S + d.o_cpos;
    uint32_t carry = 0;
    for (uint64_t s0 = 0; s0 < d.S; s0 += kLBig) {
        const uint64_t s = s0 + tid;
        const uint32_t v = (s < d.S && !iblk_dead(S, d, s, g.Bm) && tkey[s] != kInf) ? (uint32_t)__popc(info[s] & 3u) : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kLBig>(v, part, tot);
        if (s < d.S) cpos[s] = carry + ex;
        carry += tot;
    }
}

__global__ __launch_bounds__(kLB) void k_large_order(mul_large_args g) {
    const large_desc& d = g.desc[blockIdx.y];
    if (d.direct) return;
    uint32_t* S = g.scratch;
    const uint32_t* cnt = S + d.o_cnt;
    if (cnt[kCntInvalid]) return;
    const bool canonical = cnt[kCntCanonical] != 0;
    const uint32_t Bm = g.Bm, LB = d.LB, nB = d.nB;
    const uint64_t pr = d.pair;
    const uint64_t aeo = g.A.e_off[pr], beo = g.B.e_off[pr];
    const uint32_t* tkey = S + d.o_tkey;
    const uint32_t* info = S + d.o_info;
    const uint32_t* tb = S + d.o_tb;
    const uint32_t* within = S + d.o_within;
    const uint32_t* etot = S + d.o_etot;
    const unsigned long long* bpack = (const unsigned long long*)w64(S, d.o_bmask);
    const uint32_t* cpos = S + d.o_cpos;
    uint32_t* order = S + d.o_order;
    uint32_t* hpos = S + d.o_hpos;
    const uint32_t* ghead = group_heads(g, d);
    const bool ib = d.iblk && !cnt[kCntIFail];
    if (ib && !canonical && !cnt[kCntIShared]) return;   // k_large_write_ranges
    const uint32_t* icnt = S + d.o_icnt;
    const ulonglong2* imask = (const ulonglong2*)(S + d.o_imask);
    const uint64_t m = d.nb_m;
    // iblk: edges emitted before the emit time (i, j) inside A edge i's range, by probing its later
    // times (i, j'): the key slot of (i, j') is known from the two edges, and (i, j') is an emit time
    // when it is that key's first-insert time and the key is alone in its bucket or leads it
    auto probe_rank = [&](uint32_t i, uint32_t j) {
        const uint64_t ma = g.A.meta[aeo + i];
        const uint32_t sa = meta_layer(ma) * LB, ia = meta_idx(ma);
        uint32_t w = 0;
        for (uint32_t j2 = j + 1; j2 < nB; ++j2) {
            const uint64_t mb = g.B.meta[beo + j2];
            const uint64_t s2 = (uint64_t)(sa + meta_layer(mb)) * Bm + mod_small(ia + meta_idx(mb), Bm);
            const uint32_t t2 = i * nB + j2;
            if (tkey[s2] != t2) continue;
            if (ghead[s2] == 0u) w += __popc(info[s2] & 3u);
            else if (tb[s2] == t2) w += etot[s2];
        }
        return w;
    };
    for (uint64_t s = (uint64_t)blockIdx.x * kLB + threadIdx.x; s < d.S; s += (uint64_t)gridDim.x * kLB) {
        if (iblk_dead(S, d, s, Bm)) continue;
        const uint32_t ts = tkey[s];
        if (ts == kInf) continue;
        const uint32_t inf = info[s];
        const uint32_t eb = inf & 3u;
        if (!eb) continue;
        const bool lone = ghead && ghead[s] == 0u;   // its own bucket leader, nothing before it
        if (ib) {
            uint32_t hp, j0;
            const uint32_t i0 = lone ? div_small(ts, nB, m, j0) : 0u;
            const ulonglong2 mk = lone ? imask[i0] : make_ulonglong2(0ull, 0ull);
            if (lone && !(mk.x >> 63)) {   // a range without shared keys: rank from its masks
                const unsigned long long above = (~0ull << (j0 + 1)) & ~(1ull << 63);
                hp = icnt[i0] + (uint32_t)__popcll(mk.x & above) + (uint32_t)__popcll(mk.y & above);
            } else {
                const uint32_t tu = lone ? ts : tb[s];
                uint32_t j;
                const uint32_t i = div_small(tu, nB, m, j);
                hp = icnt[i] + probe_rank(i, j) + (lone ? 0u : within[s]);
            }
            const uint32_t p = canonical ? cpos[s] : hp;
            const uint32_t s32 = (uint32_t)s;
            if (eb & 1u) {
                order[p] = s32 << 1;
                if (canonical) hpos[p] = hp;
            }
            if (eb & 2u) {
                const uint32_t o = eb & 1u;
                order[p + o] = (s32 << 1) | 1u;
                if (canonical) hpos[p + o] = hp + o;
            }
            continue;
        }
        const uint32_t t = lone ? ts : tb[s], blk = t >> 4, bit = t & 15u;
        const unsigned long long v = bpack[blk];
        // edge codes of the leaders later in this block (2 bits per time): 1 and 2 are their edge
        // counts; 3 (buckets of 3+ edges) is resolved from the leader's slot, found from its
        // (i, j) = (t / |B.E|, t % |B.E|)
        const uint64_t codes = (v & 0xFFFFFFFFull) >> (2u * bit + 2u);
        const uint64_t esc = codes & (codes >> 1) & 0x5555555555555555ull;
        uint32_t hp = (uint32_t)(v >> 32) + (lone ? 0u : within[s]) + (uint32_t)__popcll(codes & 0x5555555555555555ull) +
                      2u * (uint32_t)__popcll(codes & 0xAAAAAAAAAAAAAAAAull) - 3u * (uint32_t)__popcll(esc);
        uint64_t m = esc;
        while (m) {
            const uint32_t b2 = ((uint32_t)__ffsll((long long)m) - 1u) / 2u + bit + 1u;
            m &= m - 1ull;
            const uint32_t t2 = (blk << 4) | b2;
            const uint32_t i2 = t2 / nB, j2 = t2 - i2 * nB;
            const uint64_t ma = g.A.meta[aeo + i2], mb = g.B.meta[beo + j2];
            const uint64_t s2 = (uint64_t)(meta_layer(ma) * LB + meta_layer(mb)) * Bm +
                                mod_small(meta_idx(ma) + meta_idx(mb), Bm);
            hp += etot[s2];
        }
        const uint32_t p = canonical ? cpos[s] : hp;
        const uint32_t s32 = (uint32_t)s;
        if (eb & 1u) {
            order[p] = s32 << 1;
            if (canonical) hpos[p] = hp;
        }
        if (eb & 2u) {
            const uint32_t o = eb & 1u;
            order[p + o] = (s32 << 1) | 1u;
            if (canonical) hpos[p + o] = hp + o;
        }
    }
}

__global__ __launch_bounds__(kLB) void k_large_write(mul_large_args g) {
    const large_desc& d = g.desc[blockIdx.y];
    if (d.direct) return;
    uint32_t* S = g.scratch;
    const uint32_t* cnt = S + d.o_cnt;
    if (cnt[kCntInvalid]) return;
    const uint32_t total = cnt[kCntTotal];
    const bool canonical = cnt[kCntCanonical] != 0;
    if (d.iblk && !cnt[kCntIFail] && !canonical && !cnt[kCntIShared]) return;   // k_large_write_ranges
    const uint32_t Bm = g.Bm, base = d.LA + d.LB;
    const uint64_t ceo = g.C.e_off[d.pair];
    const uint32_t* order = S + d.o_order;
    const uint32_t* hpos = S + d.o_hpos;
    const uint32_t* remap = S + d.o_used;
    const ulonglong2* sums = (const ulonglong2*)(S + d.o_sums);
    for (uint32_t p = blockIdx.x * kLB + threadIdx.x; p < total; p += gridDim.x * kLB) {
        const uint32_t e = order[p];
        const uint32_t s = e >> 1, ch = e & 1u;
        const uint32_t lp = s / Bm, r = s - lp * Bm;
        const ulonglong2 w = sums[2 * (uint64_t)s + ch];
        g.C.meta[ceo + p] = make_meta(remap[base + lp], r, ch);
        g.C.w_lo[ceo + p] = w.x;
        g.C.w_hi[ceo + p] = w.y;
        if (g.salt_pos) g.salt_pos[ceo + p] = canonical ? hpos[p] : p;
    }
}

// iblk pairs without shared buckets, hash order: the edges are written range by range. A edge
// i's keys take positions [off(i), off(i) + cnt(i)), and off decreases with i, so ranges in DESCENDING
// i are consecutive in the output. A wave takes 64 ranges (lane l: i = nA - 1 - (64 c + l)), scans
// their edge counts and writes its positions coalesced: position q of the chunk finds its lane
// (binary search over the scanned counts) and its key inside the range (j DESC; P before M: the
// k-th edge sits below the highest bit x with popc(P >> x) + popc(M >> x) <= k), the key slot from
// (A edge i, B edge j), and gathers its sum. No order array, no per-slot pass (k_large_order).
__global__ __launch_bounds__(kLB) void k_large_write_ranges(mul_large_args g) {
    __shared__ uint32_t bjt[64];   // B edge j: idx | layer << 16
    const large_desc& d = g.desc[blockIdx.y];
    if (d.direct) return;
    uint32_t* S = g.scratch;
    const uint32_t* cnt = S + d.o_cnt;
    if (cnt[kCntInvalid] || !d.iblk || cnt[kCntIFail] || cnt[kCntCanonical] || cnt[kCntIShared]) return;
    const uint32_t Bm = g.Bm, LB = d.LB, nA = d.nA, nB = d.nB, base = d.LA + d.LB;
    const uint64_t pr = d.pair;
    const uint64_t aeo = g.A.e_off[pr], beo = g.B.e_off[pr], ceo = g.C.e_off[pr];
    if (threadIdx.x < nB) {
        const uint64_t mb = g.B.meta[beo + threadIdx.x];
        bjt[threadIdx.x] = meta_idx(mb) | meta_layer(mb) << 16;
    }
    __syncthreads();
    const uint32_t* off = S + d.o_icnt;
    const ulonglong2* imask = (const ulonglong2*)(S + d.o_imask);
    const uint32_t* remap = S + d.o_used;
    const ulonglong2* sums = (const ulonglong2*)(S + d.o_sums);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nch = (nA + 63u) >> 6;
    for (uint32_t c = blockIdx.x * (kLB / 64) + (threadIdx.x >> 6); c < nch; c += gridDim.x * (kLB / 64)) {
        const uint32_t r = c * 64u + lane;
        const bool live = r < nA;
        const uint32_t i = live ? nA - 1u - r : 0u;
        // the range's edge count from the offsets (off[i - 1] - off[i], the total for i = 0); the
        // masks and the A edge are read only for ranges that hold keys
        const uint32_t oi = live ? off[i] : 0u;
        const uint32_t E = live ? (i ? off[i - 1] : cnt[kCntTotal]) - oi : 0u;
        const ulonglong2 mk = E ? imask[i] : make_ulonglong2(0ull, 0ull);
        const uint32_t o0 = off[nA - 1u - c * 64u];   // the chunk's first position (lane 0's range)
        const uint64_t ma = E ? g.A.meta[aeo + i] : 0ull;
        const uint32_t la_idx = meta_idx(ma) | meta_layer(ma) << 16;
        const uint32_t incl = wave_incl_scan_u32(E);
        const uint32_t T = __builtin_amdgcn_readlane(incl, 63);
        // position q of the chunk -> key slot s and channel; every lane takes part in the bpermutes
        auto resolve = [&](uint32_t q, uint64_t& s, uint32_t& ch, uint32_t& lp, uint32_t& rr) {
            // lane l of the range holding q: the first lane whose inclusive count exceeds q
            uint32_t l = 0;
#pragma unroll
            for (uint32_t b = 32; b; b >>= 1) {
                const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((l + b - 1u) << 2), (int)incl);
                if (v <= q) l += b;
            }
            l = min(l, 63u);
            const int bl = (int)(l << 2);
            const uint32_t il = (uint32_t)__builtin_amdgcn_ds_bpermute(bl, (int)incl) -
                                (uint32_t)__builtin_amdgcn_ds_bpermute(bl, (int)E);
            const uint64_t mp = (uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(bl, (int)(uint32_t)mk.x) |
                                (uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(bl, (int)(uint32_t)(mk.x >> 32)) << 32;
            const uint64_t mm = (uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(bl, (int)(uint32_t)mk.y) |
                                (uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(bl, (int)(uint32_t)(mk.y >> 32)) << 32;
            const uint32_t ai = (uint32_t)__builtin_amdgcn_ds_bpermute(bl, (int)la_idx);
            const uint32_t k = q - il;   // edge k of the range (q < T)
            // edges of keys at bits >= y: A(y) = popc(mp >> y) + popc(mm >> y), non-increasing; the
            // key holding edge k is the largest j with A(j) > k
            uint32_t j = 0;
#pragma unroll
            for (uint32_t b = 32; b; b >>= 1) {
                const uint32_t y = j + b;
                if ((uint32_t)__popcll(mp >> y) + (uint32_t)__popcll(mm >> y) > k) j = y;
            }
            const uint32_t fa = j == 63u ? 0u : (uint32_t)__popcll(mp >> (j + 1u)) + (uint32_t)__popcll(mm >> (j + 1u));
            const uint32_t hasP = (uint32_t)(mp >> j) & 1u;
            ch = (k - fa == 0u && hasP) ? 0u : 1u;   // a key emits P before M
            const uint32_t bj = bjt[j];
            lp = (ai >> 16) * LB + (bj >> 16);
            rr = mod_small((ai & 0xFFFFu) + (bj & 0xFFFFu), Bm);
            s = (uint64_t)lp * Bm + rr;
        };
        // two positions per lane and round: both gathers in flight before the stores
        for (uint32_t q0 = 0; q0 < T; q0 += 128u) {   // wave-uniform
            uint64_t s[2];
            uint32_t ch[2], lp[2], rr[2];
            ulonglong2 w[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const uint32_t q = q0 + 64u * (uint32_t)u + lane;
                resolve(min(q, T - 1u), s[u], ch[u], lp[u], rr[u]);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) w[u] = sums[2 * s[u] + ch[u]];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const uint32_t q = q0 + 64u * (uint32_t)u + lane;
                if (q >= T) break;
                const uint64_t p = ceo + o0 + q;
                g.C.meta[p] = make_meta(remap[base + lp[u]], rr[u], ch[u]);
                g.C.w_lo[p] = w[u].x;
                g.C.w_hi[p] = w[u].y;
                if (g.salt_pos) g.salt_pos[p] = o0 + q;
            }
        }
    }
}

}  // namespace

// the stages of this file a deep sub-batch shares with the others (k_large_deep.hip launches its own
// lists and layers kernels between them): its pairs are never iblk, direct or in a static group
void launch_large_init(const mul_large_args& a, hipStream_t st) {
    hipLaunchKernelGGL(k_large_init, dim3(grid_x(a.max_zero > a.max_S ? a.max_zero : a.max_S, kLB * 4, 4096), a.nl),
                       dim3(kLB), 0, st, a);
}

void launch_large_emit(const mul_large_args& a, hipStream_t st) {
    const unsigned nl = a.nl;
    const unsigned gs = grid_x(a.max_S, kLB * 2, 4096);
    hipLaunchKernelGGL(k_large_link, dim3(gs, nl), dim3(kLB), 0, st, a);
    hipLaunchKernelGGL(k_large_rank, dim3(gs, nl), dim3(kLB), 0, st, a);
    hipLaunchKernelGGL(k_large_scan, dim3(nl), dim3(kLBig), 0, st, a);
    hipLaunchKernelGGL(k_large_order, dim3(gs, nl), dim3(kLB), 0, st, a);
    hipLaunchKernelGGL(k_large_write, dim3(grid_x(a.max_capE, kLB * 2, 4096), nl), dim3(kLB), 0, st, a);
}

hipError_t launch_ct_mul_large(const mul_large_args& a, hipStream_t st) {
    if (!a.nl) return hipSuccess;
    if (a.deep) {   // (the host runtime launches the stages itself, two of them under their timing names)
        hipError_t e = hipSuccess;
        for (int stage = 0; stage < kDeepStages && e == hipSuccess; ++stage) e = launch_ct_mul_large_deep(a, stage, st);
        return e;
    }
    if (a.Bm > kBmax || a.max_lay > kLargeLayersMax) return hipErrorInvalidValue;
    const unsigned nl = a.nl;
    hipLaunchKernelGGL(k_large_init, dim3(grid_x(a.max_zero > a.max_S ? a.max_zero : a.max_S, kLB * 4, 4096), nl),
                       dim3(kLB), 0, st, a);
    hipLaunchKernelGGL(k_large_lists, dim3(nl), dim3(kLBig), (size_t)a.max_lay * 4, st, a);
    if (a.any_direct && a.n_la && a.max_la_wg) {
        // direct pairs: presence counts, offsets, compact_layers, then products straight to C
        mul_large_args b = a;
        launch_large_direct_count(b, st);
        b.layers_direct = 1;
        hipLaunchKernelGGL(k_large_layers, dim3(nl), dim3(kLBig), (size_t)a.max_lay * 4, st, b);
        launch_large_direct_products(b, st);
        if (a.all_direct) return hipGetLastError();
    }
    launch_large_products(a, st);
    hipLaunchKernelGGL(k_large_layers, dim3(nl), dim3(kLBig), (size_t)a.max_lay * 4, st, a);
    const unsigned gs = grid_x(a.max_S, kLB * 2, 4096);
    // a batch of iblk pairs runs rank / order / write only for the few that share buckets, need the
    // canonical order or fell back: 1/16 of the workgroups (grid-stride loops; an empty workgroup per
    // 512 slots cost 5 ms per sub-batch and kernel at cfg 4's depth 8)
    const unsigned sh = a.all_iblk ? 4u : 0u;
    const unsigned gsr = (gs + (1u << sh) - 1u) >> sh;
    if (a.any_dyn) hipLaunchKernelGGL(k_large_link, dim3(gs, nl), dim3(kLB), 0, st, a);
    hipLaunchKernelGGL(k_large_rank, dim3(gsr, nl), dim3(kLB), 0, st, a);
    hipLaunchKernelGGL(k_large_scan, dim3(nl), dim3(kLBig), 0, st, a);
    hipLaunchKernelGGL(k_large_order, dim3(gsr, nl), dim3(kLB), 0, st, a);
    const unsigned gw = grid_x(a.max_capE, kLB * 2, 4096);
    hipLaunchKernelGGL(k_large_write, dim3((gw + (1u << sh) - 1u) >> sh, nl), dim3(kLB), 0, st, a);
    if (a.max_nA) hipLaunchKernelGGL(k_large_write_ranges, dim3(grid_x(a.max_nA, kLB, 4096), nl), dim3(kLB), 0, st, a);
    return hipGetLastError();
}

}  // namespace pvhip
