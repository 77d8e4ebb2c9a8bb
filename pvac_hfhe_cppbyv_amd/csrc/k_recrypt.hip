// k_recrypt.hip — the parts of ct_recrypt (ops/recrypt.hpp:26-41) that touch every sigma row:
//   k_sigma_popcount  sigma_density's numerator (ops/encrypt.hpp:29-37): popcnt over a cipher's rows
//   k_ubk_apply       ubk_apply (crypto/matrix.hpp:167-188, 306-310): out[inv[src]] = in[src] per row
//   k_compact_small   compact_edges + compact_layers (ops/encrypt.hpp:39-104) for a batch, one
//                     workgroup per cipher whose key space |L| 2B fits kCompactSmallCells LDS words
// A cipher above the bound takes launch_add_merge with an empty B (k_add_merge.hip).
#include "common.hpp"
#include "compact_layers.hpp"

#include <algorithm>

namespace pvhip {
namespace {

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---------------------------------------------------------------- sigma_popcount
// Workgroup blockIdx.x serves split s = blockIdx.x % splits of cipher blockIdx.x / splits: a
// contiguous share of the cipher's sigma words, streamed once (16-byte loads when the rows are
// dense and aligned), one atomic add per workgroup into ones[i] (zeroed by the host).
constexpr int kPopBlock = 256;

__global__ __launch_bounds__(kPopBlock) void k_sigma_popcount(pvac_ct_batch X, uint32_t mw, uint32_t splits, int wide,
                                                              unsigned long long* ones) {
    __shared__ unsigned long long part[kPopBlock / 64];
    const uint64_t i = blockIdx.x / splits;
    const uint32_t s = blockIdx.x % splits;
    const uint64_t ne = X.e_cnt[i];
    if (!ne) return;
    const uint32_t sw = X.sigma_words;
    const uint64_t* base = X.sigma + X.e_off[i] * sw;
    unsigned long long acc = 0;
    if (wide) {   // mw == sw, sw even, base 16-byte aligned: the rows are one dense range
        const uint64_t units = ne * (sw / 2);
        const uint64_t per = (units + splits - 1) / splits;
        const uint64_t lo = min(units, (uint64_t)s * per), hi = min(units, lo + per);
        const u64x2* p = (const u64x2*)base;
        for (uint64_t u = lo + threadIdx.x; u < hi; u += kPopBlock) {
            const u64x2 v = __builtin_nontemporal_load(p + u);
            acc += (unsigned)__popcll(v.x) + (unsigned)__popcll(v.y);
        }
    } else {      // rows of mw used words at a stride of sw
        const uint64_t per = (ne + splits - 1) / splits;
        const uint64_t lo = min(ne, (uint64_t)s * per), hi = min(ne, lo + per);
        const uint64_t words = (hi - lo) * mw;
        for (uint64_t t = threadIdx.x; t < words; t += kPopBlock) {
            const uint64_t r = t / mw;
            acc += (unsigned)__popcll(base[(lo + r) * sw + (t - r * mw)]);
        }
    }
    acc = wave_sum_u64(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot = 0;
        for (int w = 0; w < kPopBlock / 64; ++w) tot += part[w];
        if (tot) atomicAdd(&ones[i], tot);
    }
}

// ---------------------------------------------------------------- ubk_apply
// Gather form: out bit j = in bit perm[j] (perm[inv[src]] = src, built by the host). One wave per
// edge row: the row is staged in LDS, lane l owns the output bits 64 w + l, and the 64-bit ballot of
// "source bit set" is output word w; lane w mod 64 keeps it, so every 64 words leave as one
// coalesced store. perm is loaded into LDS once per (persistent) workgroup. The loops' trip counts
// are workgroup-uniform, so the barriers are too.
constexpr int kUbkWaves = 4;

__global__ __launch_bounds__(64 * kUbkWaves) void k_ubk_apply(pvac_ct_batch X, const uint32_t* perm, uint32_t m_bits,
                                                              uint32_t mw, uint32_t splits, uint64_t items,
                                                              const uint32_t* active) {
    extern __shared__ uint64_t ubk_lds[];   // [kUbkWaves][mw] staged rows, then [64 mw] u32 perm
    uint32_t* lperm = (uint32_t*)(ubk_lds + (size_t)kUbkWaves * mw);
    for (uint32_t t = threadIdx.x; t < 64u * mw; t += 64 * kUbkWaves) lperm[t] = t < m_bits ? perm[t] : 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t* row = ubk_lds + (size_t)wave * mw;
    const uint32_t* row32 = (const uint32_t*)row;
    const uint32_t sw = X.sigma_words;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint64_t i = item / splits;
        const uint32_t s = (uint32_t)(item % splits);
        uint64_t ne = X.e_cnt[i];
        if (active && !active[i]) ne = 0;
        const uint64_t per = (ne + splits - 1) / splits;
        const uint64_t lo = min(ne, (uint64_t)s * per), hi = min(ne, lo + per);
        const uint64_t eo = X.e_off[i];
        for (uint64_t r0 = lo; r0 < hi; r0 += kUbkWaves) {
            const uint64_t r = r0 + wave;
            const bool live = r < hi;
            uint64_t* g = X.sigma + (eo + r) * sw;
            if (live)
                for (uint32_t w = lane; w < mw; w += 64) row[w] = g[w];
            __syncthreads();
            if (live) {
                uint64_t mine = 0;
                for (uint32_t w = 0; w < mw; ++w) {
                    const uint32_t src = lperm[64u * w + lane];
                    const uint32_t bit = src != 0xFFFFFFFFu ? (row32[src >> 5] >> (src & 31u)) & 1u : 0u;
                    const uint64_t b = __ballot(bit);
                    if (lane == (w & 63u)) mine = b;
                    if ((w & 63u) == 63u || w + 1 == mw) {
                        const uint32_t w0 = w & ~63u;
                        if (w0 + lane <= w) g[w0 + lane] = mine;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// The reference's m_bits = 8192 (128 words per row). The loop above waits for two dependent LDS
// reads per position, so it is bound by LDS latency. Here the lane's 128 perm entries (13 bits
// each) live in 64 registers, a wave permutes kUbkRows rows together (the decode of a position is
// shared), and the source words of kUbkGroup positions x kUbkRows rows are requested before the first
// is used, so the reads overlap instead of being waited for one by one.
constexpr int kUbkRows = 4;
constexpr int kUbkGroup = 8;

__global__ __launch_bounds__(64 * kUbkWaves, 2) void k_ubk_apply_128(pvac_ct_batch X, const uint32_t* perm,
                                                                     uint32_t splits, uint64_t items,
                                                                     const uint32_t* active) {
    __shared__ uint64_t rows[kUbkWaves][kUbkRows][128];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t pr[64];   // positions 2 k and 2 k + 1 in the halves of pr[k]
#pragma unroll
    for (int k = 0; k < 64; ++k) pr[k] = perm[64 * (2 * k) + lane] | (perm[64 * (2 * k + 1) + lane] << 16);
    const char* mine_rows = (const char*)&rows[wave][0][0];
    const uint32_t sw = X.sigma_words;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint64_t i = item / splits;
        const uint32_t s = (uint32_t)(item % splits);
        uint64_t ne = X.e_cnt[i];
        if (active && !active[i]) ne = 0;
        const uint64_t per = (ne + splits - 1) / splits;
        const uint64_t lo = min(ne, (uint64_t)s * per), hi = min(ne, lo + per);
        uint64_t* const g0 = X.sigma + X.e_off[i] * sw;
        for (uint64_t r0 = lo; r0 < hi; r0 += kUbkWaves * kUbkRows) {   // workgroup-uniform trip count
            const uint64_t r = r0 + (uint64_t)wave * kUbkRows;
#pragma unroll
            for (int j = 0; j < kUbkRows; ++j)
                if (r + j < hi) {
                    const uint64_t* g = g0 + (r + j) * sw;
                    rows[wave][j][lane] = g[lane];
                    rows[wave][j][lane + 64] = g[lane + 64];
                }
            __syncthreads();
            uint32_t out_lo[kUbkRows], out_hi[kUbkRows];
#pragma unroll
            for (int j = 0; j < kUbkRows; ++j) out_lo[j] = out_hi[j] = 0;
#pragma unroll
            for (int w0 = 0; w0 < 128; w0 += kUbkGroup) {
                uint32_t src[kUbkGroup], word[kUbkGroup][kUbkRows];
#pragma unroll
                for (int k = 0; k < kUbkGroup; ++k) {
                    const int w = w0 + k;
                    uint32_t q = pr[w >> 1];
                    asm volatile("" : "+v"(q));   // decode here, per use: hoisted out of the row loop it costs 256 registers
                    src[k] = (w & 1) ? q >> 16 : q & 0xFFFFu;
                    const uint32_t addr = (src[k] >> 5) << 2;
#pragma unroll
                    for (int j = 0; j < kUbkRows; ++j) word[k][j] = *(const uint32_t*)(mine_rows + j * 1024 + addr);
                }
#pragma unroll
                for (int k = 0; k < kUbkGroup; ++k) {
                    const int w = w0 + k;
                    const bool keeper = lane == (uint32_t)(w & 63);   // the lane that stores output word w
#pragma unroll
                    for (int j = 0; j < kUbkRows; ++j) {
                        const uint64_t b = __ballot((word[k][j] >> (src[k] & 31u)) & 1u);
                        out_lo[j] = keeper ? (uint32_t)b : out_lo[j];
                        out_hi[j] = keeper ? (uint32_t)(b >> 32) : out_hi[j];
                    }
                }
                if (((w0 + kUbkGroup - 1) & 63) == 63) {
#pragma unroll
                    for (int j = 0; j < kUbkRows; ++j)
                        if (r + j < hi)
                            g0[(r + j) * sw + (w0 & ~63) + lane] = (uint64_t)out_lo[j] | ((uint64_t)out_hi[j] << 32);
                }
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------- compact (small key spaces)
// One LDS word per cell (cell id = (layer B + idx) 2 + ch, the output order): the first edge of the
// cell in input order (30 bits), a flag "more than one edge", a flag "kept".
constexpr int kCsBlock = 512;
constexpr uint32_t kCsNone = 0x3FFFFFFFu;    // first-edge field of an empty cell
constexpr uint32_t kCsKeep = 0x40000000u;
constexpr uint32_t kCsMulti = 0x80000000u;
constexpr uint32_t kCsBadKey = 0xFFFFFFFFu;
static_assert(kCompactSmallCells / 64 <= kCsBlock, "one 64-cell group per thread in the position scan");
static_assert(kCompactSmallEdges <= kCsNone, "edge indices fit the first-edge field");

struct cs_src {
    const uint64_t *m, *lo, *hi, *sg;   // the cipher's edge arrays at its offset
    uint32_t ne, L, Bm, sw;
};

__device__ __forceinline__ uint32_t cs_key(const cs_src& x, uint32_t e) {
    const uint64_t m = x.m[e];
    const uint32_t lid = meta_layer(m), idx = meta_idx(m);
    const uint32_t ch = meta_ch(m) != 0 ? 1u : 0u;   // anything but SGN_P aggregates as M (encrypt.hpp:48-56)
    // out-of-range references (undefined in the reference) are dropped, as k_merge_keys does
    return (lid < x.L && idx < x.Bm) ? (lid * x.Bm + idx) * 2u + ch : kCsBadKey;
}

// the cell's sequential fp_add chain from 0 in edge order (encrypt.hpp:46-56), quirks included
__device__ __forceinline__ fp cs_fold(const cs_src& x, uint32_t cell, uint32_t v) {
    const uint32_t first = v & kCsNone;
    fp acc = fp_add(fp{0, 0}, fp{x.lo[first], x.hi[first]});
    if (v & kCsMulti)
        for (uint32_t e = first + 1; e < x.ne; ++e)
            if (cs_key(x, e) == cell) acc = fp_add(acc, fp{x.lo[e], x.hi[e]});
    return acc;
}

// word w of the cell's sigma XOR (all lanes of a wave call it with the same cell)
__device__ __forceinline__ uint64_t cs_sigma_word(const cs_src& x, uint32_t cell, uint32_t v, uint32_t w) {
    const uint32_t first = v & kCsNone;
    uint64_t s = x.sg[(uint64_t)first * x.sw + w];
    if (v & kCsMulti)
        for (uint32_t e = first + 1; e < x.ne; ++e)
            if (cs_key(x, e) == cell) s ^= x.sg[(uint64_t)e * x.sw + w];
    return s;
}

__global__ __launch_bounds__(kCsBlock) void k_compact_small(pvac_ct_batch X, pvac_ct_batch C, const uint8_t* cls,
                                                            uint32_t Bm, uint32_t mw, int wide) {
    extern __shared__ uint32_t cell[];                     // [G * 64]
    __shared__ uint32_t lay[kCompactSmallLayers];          // used flags, then the layer remap
    __shared__ uint32_t gbase[kCompactSmallCells / 64];    // kept cells per 64-cell group, then their scan
    __shared__ uint32_t part[kCsBlock / 64];
    __shared__ uint32_t changed;
    const uint64_t i = blockIdx.x;
    if (cls[i] != PAIR_SMALL) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t L = (uint32_t)X.l_cnt[i];
    const uint64_t xlo = X.l_off[i], clo = C.l_off[i], xeo = X.e_off[i], ceo = C.e_off[i];
    cs_src x;
    x.ne = (uint32_t)X.e_cnt[i];
    x.L = L;
    x.Bm = Bm;
    x.sw = X.sigma_words;
    x.m = X.meta + xeo;
    x.lo = X.w_lo + xeo;
    x.hi = X.w_hi + xeo;
    x.sg = X.sigma + xeo * x.sw;
    if (x.ne == 0 || L == 0) {   // no edge: compact_layers drops every layer
        if (tid == 0) {
            C.l_cnt[i] = 0;
            C.e_cnt[i] = 0;
        }
        return;
    }
    const uint32_t K = L * 2u * Bm, G = (K + 63u) / 64u;
    volatile uint32_t* vcell = cell;
    for (uint32_t c = tid; c < G * 64u; c += kCsBlock) cell[c] = kCsNone;
    for (uint32_t l = tid; l < L; l += kCsBlock) lay[l] = 0;
    __syncthreads();
    // 1. first edge of every cell, then the cells with more edges than that one
    for (uint32_t e = tid; e < x.ne; e += kCsBlock) {
        const uint32_t k = cs_key(x, e);
        if (k != kCsBadKey) atomicMin(&cell[k], e);
    }
    __syncthreads();
    for (uint32_t e = tid; e < x.ne; e += kCsBlock) {
        const uint32_t k = cs_key(x, e);
        if (k != kCsBadKey && (vcell[k] & kCsNone) != e) atomicOr(&cell[k], kCsMulti);
    }
    __syncthreads();
    // 2. keep flags: lane <-> cell in groups of 64. A cell is dropped only when its sum and its sigma
    //    XOR are both zero (encrypt.hpp:59); the sigma is read only for a zero sum, by the whole wave
    for (uint32_t g = wave; g < G; g += kCsBlock / 64) {
        const uint32_t c = 64u * g + lane;
        const uint32_t v = cell[c];
        const bool has = (v & kCsNone) != kCsNone;
        bool keep = has && fp_nonzero(cs_fold(x, c, v));
        uint64_t zm = __ballot(has && !keep);
        while (zm) {
            const uint32_t b = (uint32_t)__builtin_ctzll(zm);
            zm &= zm - 1;
            const uint32_t cb = 64u * g + b, vb = cell[cb];
            uint64_t any = 0;
            for (uint32_t w = lane; w < mw; w += 64) any |= cs_sigma_word(x, cb, vb, w);
            if (__ballot(any != 0) != 0 && lane == b) keep = true;
        }
        if (keep) {
            cell[c] = v | kCsKeep;
            lay[c / (2u * Bm)] = 1;
        }
        const uint64_t km = __ballot(keep);
        if (lane == 0) gbase[g] = (uint32_t)__popcll(km);
    }
    __syncthreads();
    // 3. compact_layers (encrypt.hpp:73-104): PROD parents of used layers until stable, then the remap
    const pvac_layer* xl = X.layers + xlo;
    block_close<kCsBlock>(lay, L, &changed, [&](uint32_t l, uint32_t& rule, uint32_t& pa, uint32_t& pb) {
        rule = xl[l].rule; pa = xl[l].pa; pb = xl[l].pb;
    });
    const uint32_t kept = block_remap<kCsBlock>(lay, lay, L, part);
    const bool identity = kept == L;
    for (uint32_t l = tid; l < L; l += kCsBlock) {
        const uint32_t to = lay[l];
        if (to == kDropped) continue;
        const pvac_layer& y = xl[l];   // field by field: a local copy of the record goes to scratch
        pvac_layer& z = C.layers[clo + to];
        uint32_t pa = y.pa, pb = y.pb;
        if (!identity && y.rule == 1) {
            pa = pa < L ? lay[pa] : kDropped;
            pb = pb < L ? lay[pb] : kDropped;
        }
        z.rule = y.rule;
        z.pa = pa;
        z.pb = pb;
        z.pad = y.pad;
        z.ztag = y.ztag;
        z.nonce_lo = y.nonce_lo;
        z.nonce_hi = y.nonce_hi;
    }
    // 4. output positions: exclusive scan of the groups' kept counts (G <= kCsBlock)
    uint32_t total;
    const uint32_t gv = tid < G ? gbase[tid] : 0u;
    const uint32_t gx = block_exclusive_scan<kCsBlock>(gv, part, total);
    if (tid < G) gbase[tid] = gx;
    if (tid == 0) {
        C.l_cnt[i] = kept;
        C.e_cnt[i] = total;
    }
    __syncthreads();
    // 5. write: (meta, w) by the cell's lane (consecutive positions across the lanes), the 1 KiB
    //    sigma rows by the whole wave, streamed past the caches
    const uint32_t csw = C.sigma_words;
    for (uint32_t g = wave; g < G; g += kCsBlock / 64) {
        const uint32_t c = 64u * g + lane;
        const uint32_t v = cell[c];
        const bool keep = (v & kCsKeep) != 0;
        const uint64_t km = __ballot(keep);
        if (!km) continue;
        const uint32_t base = gbase[g];
        if (keep) {
            const uint32_t pos = base + (uint32_t)__popcll(km & ((1ull << lane) - 1ull));
            const fp s = cs_fold(x, c, v);
            const uint32_t lid = c / (2u * Bm), rem = c - lid * 2u * Bm;
            __builtin_nontemporal_store((unsigned long long)make_meta(lay[lid], rem >> 1, rem & 1u),
                                        (unsigned long long*)C.meta + ceo + pos);
            __builtin_nontemporal_store((unsigned long long)s.lo, (unsigned long long*)C.w_lo + ceo + pos);
            __builtin_nontemporal_store((unsigned long long)s.hi, (unsigned long long*)C.w_hi + ceo + pos);
        }
        uint64_t rest = km;
        uint32_t pos = base;
        while (rest) {
            const uint32_t b = (uint32_t)__builtin_ctzll(rest);
            const uint32_t cb = 64u * g + b, vb = cell[cb];
            if (wide && !(vb & kCsMulti)) {
                // single-edge cells, 128-word rows: 16 bytes per lane, up to four rows in flight
                uint32_t src[4];
                int nr = 0;
                uint64_t r2 = rest;
#pragma unroll
                for (int k = 0; k < 4; ++k) {   // unrolled: src[] and t[] stay in registers
                    src[k] = 0;
                    if (nr != k || !r2) continue;
                    const uint32_t vv = cell[64u * g + (uint32_t)__builtin_ctzll(r2)];
                    if (vv & kCsMulti) continue;
                    src[k] = vv & kCsNone;
                    nr = k + 1;
                    r2 &= r2 - 1;
                }
                u64x2 t[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < nr) t[k] = __builtin_nontemporal_load((const u64x2*)(x.sg + (uint64_t)src[k] * 128u) + lane);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < nr) __builtin_nontemporal_store(t[k], (u64x2*)(C.sigma + (ceo + pos + k) * 128u) + lane);
                pos += nr;
                rest = r2;
                continue;
            }
            uint64_t* dst = C.sigma + (ceo + pos) * csw;
            for (uint32_t w = lane; w < mw; w += 64)
                __builtin_nontemporal_store((unsigned long long)cs_sigma_word(x, cb, vb, w), (unsigned long long*)dst + w);
            pos += 1;
            rest &= rest - 1;
        }
    }
}

// ---------------------------------------------------------------- compact plan
constexpr int kCpBlock = 256;
// counts -> C's offset arrays when given (scanned in place afterwards), the class of every cipher, the ids of
// those left to the merge path, and the launch maxima of the small ones
__global__ __launch_bounds__(kCpBlock) void k_compact_plan(pvac_ct_batch X, uint64_t* c_l_off, uint64_t* c_e_off,
                                                           uint32_t Bm, uint8_t* cls, uint64_t* large_ids,
                                                           plan_stats* st) {
    const uint64_t i = (uint64_t)blockIdx.x * kCpBlock + threadIdx.x;
    if (i >= X.n) return;
    const uint64_t L = X.l_cnt[i], ne = X.e_cnt[i];
    if (c_l_off) c_l_off[i] = L;
    if (c_e_off) c_e_off[i] = ne;
    const bool small = ne == 0 || L == 0 ||
                       (L <= kCompactSmallLayers && ne <= kCompactSmallEdges && L * 2u * Bm <= kCompactSmallCells);
    cls[i] = small ? PAIR_SMALL : PAIR_LARGE;
    if (small) {
        if (ne && L) atomicMax(&st->max_keys, (unsigned int)(L * 2u * Bm));
    } else {
        large_ids[atomicAdd(&st->n_large, 1ull)] = i;
    }
    atomicMax(&st->max_layers, (unsigned int)min(L, (uint64_t)0xFFFFFFFFu));
}

// 8 words per listed cipher: id, |L|, |E|, X's edge offset, C's edge offset (after the scans)
__global__ __launch_bounds__(kCpBlock) void k_compact_gather(pvac_ct_batch X, const uint64_t* c_e_off,
                                                             const uint64_t* ids, uint64_t n, uint64_t* out) {
    const uint64_t k = (uint64_t)blockIdx.x * kCpBlock + threadIdx.x;
    if (k >= n) return;
    const uint64_t i = ids[k];
    uint64_t* o = out + 8 * k;
    o[0] = i;
    o[1] = X.l_cnt[i];
    o[2] = X.e_cnt[i];
    o[3] = X.e_off[i];
    o[4] = c_e_off[i];
    o[5] = o[6] = o[7] = 0;
}

// ---------------------------------------------------------------- ct_recrypt plumbing
// output capacities |X.L| + 8 max|pool.L| and |X.E| + 8 max|pool.E| (eight ct_adds at most,
// recrypt.hpp:31-36) into C's offset arrays (scanned afterwards); C's counts start at 0
__global__ __launch_bounds__(kCpBlock) void k_recrypt_plan(pvac_ct_batch X, uint64_t max_pl, uint64_t max_pe,
                                                           pvac_ct_batch C) {
    const uint64_t i = (uint64_t)blockIdx.x * kCpBlock + threadIdx.x;
    if (i >= X.n) return;
    C.l_off[i] = X.l_cnt[i] + 8 * max_pl;
    C.e_off[i] = X.e_cnt[i] + 8 * max_pe;
    if (C.l_cnt) C.l_cnt[i] = 0;
    if (C.e_cnt) C.e_cnt[i] = 0;
}

// cipher ids[k] of X verbatim into its slots of C (an empty pool, an empty edge list: recrypt.hpp:27)
__global__ __launch_bounds__(kCpBlock) void k_recrypt_copy(pvac_ct_batch X, pvac_ct_batch C, const uint32_t* ids,
                                                           uint32_t mw) {
    const uint64_t i = ids[blockIdx.x];
    const uint64_t L = X.l_cnt[i], ne = X.e_cnt[i];
    const uint64_t xlo = X.l_off[i], clo = C.l_off[i], xeo = X.e_off[i], ceo = C.e_off[i];
    const uint64_t* ls = (const uint64_t*)(X.layers + xlo);
    uint64_t* ld = (uint64_t*)(C.layers + clo);
    for (uint64_t t = threadIdx.x; t < L * (sizeof(pvac_layer) / 8); t += kCpBlock) ld[t] = ls[t];
    for (uint64_t e = threadIdx.x; e < ne; e += kCpBlock) {
        C.meta[ceo + e] = X.meta[xeo + e];
        C.w_lo[ceo + e] = X.w_lo[xeo + e];
        C.w_hi[ceo + e] = X.w_hi[xeo + e];
    }
    for (uint64_t t = threadIdx.x; t < ne * mw; t += kCpBlock) {
        const uint64_t e = t / mw, w = t - e * mw;
        C.sigma[(ceo + e) * C.sigma_words + w] = X.sigma[(xeo + e) * X.sigma_words + w];
    }
    if (threadIdx.x == 0) {
        C.l_cnt[i] = L;
        C.e_cnt[i] = ne;
    }
}

// the counts a view's compaction wrote, back to the ciphers the view stands for
__global__ __launch_bounds__(kCpBlock) void k_scatter_counts(const uint64_t* l_cnt, const uint64_t* e_cnt,
                                                             const uint32_t* ids, uint64_t m, uint64_t* c_l_cnt,
                                                             uint64_t* c_e_cnt) {
    const uint64_t k = (uint64_t)blockIdx.x * kCpBlock + threadIdx.x;
    if (k >= m) return;
    c_l_cnt[ids[k]] = l_cnt[k];
    c_e_cnt[ids[k]] = e_cnt[k];
}

}  // namespace

hipError_t launch_recrypt_plan(const pvac_ct_batch& X, uint64_t max_pl, uint64_t max_pe, pvac_ct_batch& C, hipStream_t st) {
    hipLaunchKernelGGL(k_recrypt_plan, dim3((unsigned)((X.n + kCpBlock - 1) / kCpBlock)), dim3(kCpBlock), 0, st, X, max_pl,
                       max_pe, C);
    return hipGetLastError();
}

hipError_t launch_recrypt_copy(const pvac_ct_batch& X, pvac_ct_batch& C, const uint32_t* ids, uint64_t m, uint32_t m_bits,
                               hipStream_t st) {
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_recrypt_copy, dim3((unsigned)m), dim3(kCpBlock), 0, st, X, C, ids, (m_bits + 63) / 64);
    return hipGetLastError();
}

hipError_t launch_scatter_counts(const uint64_t* l_cnt, const uint64_t* e_cnt, const uint32_t* ids, uint64_t m,
                                 uint64_t* c_l_cnt, uint64_t* c_e_cnt, hipStream_t st) {
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_scatter_counts, dim3((unsigned)((m + kCpBlock - 1) / kCpBlock)), dim3(kCpBlock), 0, st, l_cnt, e_cnt,
                       ids, m, c_l_cnt, c_e_cnt);
    return hipGetLastError();
}

hipError_t launch_sigma_popcount(const pvac_ct_batch& X, uint32_t m_bits, int num_cus, unsigned long long* ones,
                                 hipStream_t st) {
    if (!X.n) return hipSuccess;
    hipError_t e = hipMemsetAsync(ones, 0, X.n * 8, st);
    if (e != hipSuccess) return e;
    const uint32_t mw = (m_bits + 63) / 64;
    const uint64_t want = (uint64_t)num_cus * 8;
    const uint32_t splits = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((want + X.n - 1) / X.n, 1), 4096);
    if (X.n * splits > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const int wide = mw == X.sigma_words && !(mw & 1u) && ((uintptr_t)X.sigma & 15u) == 0;
    hipLaunchKernelGGL(k_sigma_popcount, dim3((unsigned)(X.n * splits)), dim3(kPopBlock), 0, st, X, mw, splits, wide, ones);
    return hipGetLastError();
}

size_t ubk_apply_lds_bytes(uint32_t m_bits) {
    const size_t mw = (m_bits + 63) / 64;
    return (size_t)kUbkWaves * mw * 8 + 64 * mw * 4;
}

hipError_t launch_ubk_apply(const pvac_ct_batch& X, const uint32_t* perm, uint32_t m_bits, const uint32_t* active,
                            int num_cus, hipStream_t st) {
    if (!X.n) return hipSuccess;
    const uint32_t mw = (m_bits + 63) / 64;
    const bool fixed = m_bits == 8192;
    // persistent workgroups: exactly as many as are resident at once, so none runs in a thin second round
    int per_cu = 0;
    hipError_t e = fixed ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_ubk_apply_128, 64 * kUbkWaves, 0)
                         : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_ubk_apply, 64 * kUbkWaves,
                                                                        ubk_apply_lds_bytes(m_bits));
    if (e != hipSuccess) return e;
    const uint64_t want = (uint64_t)num_cus * std::max(per_cu, 1);
    const uint32_t splits = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((4 * want + X.n - 1) / X.n, 1), 1024);
    const uint64_t items = X.n * splits;
    const unsigned grid = (unsigned)std::min<uint64_t>(items, want);
    if (fixed) {
        hipLaunchKernelGGL(k_ubk_apply_128, dim3(grid), dim3(64 * kUbkWaves), 0, st, X, perm, splits, items, active);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_ubk_apply, dim3(grid), dim3(64 * kUbkWaves), ubk_apply_lds_bytes(m_bits), st, X, perm, m_bits, mw,
                       splits, items, active);
    return hipGetLastError();
}

hipError_t launch_compact_plan(const pvac_ct_batch& X, pvac_ct_batch& C, uint32_t Bm, uint8_t* cls, uint64_t* large_ids,
                               plan_stats* stats, hipStream_t st) {
    hipLaunchKernelGGL(k_compact_plan, dim3((unsigned)((X.n + kCpBlock - 1) / kCpBlock)), dim3(kCpBlock), 0, st, X, C.l_off,
                       C.e_off, Bm, cls, large_ids, stats);
    return hipGetLastError();
}

hipError_t launch_compact_gather(const pvac_ct_batch& X, const pvac_ct_batch& C, const uint64_t* ids, uint64_t n,
                                 uint64_t* out, hipStream_t st) {
    hipLaunchKernelGGL(k_compact_gather, dim3((unsigned)((n + kCpBlock - 1) / kCpBlock)), dim3(kCpBlock), 0, st, X, C.e_off,
                       ids, n, out);
    return hipGetLastError();
}

hipError_t launch_compact_small(const pvac_ct_batch& X, pvac_ct_batch& C, const uint8_t* cls, uint32_t Bm, uint32_t m_bits,
                                uint32_t max_cells, hipStream_t st) {
    if (!X.n) return hipSuccess;
    if (X.n > 0x7FFFFFFFull || max_cells > kCompactSmallCells) return hipErrorInvalidValue;
    const uint32_t mw = (m_bits + 63) / 64;
    const int wide = mw == 128 && X.sigma_words == 128 && C.sigma_words == 128 && ((uintptr_t)X.sigma & 15u) == 0 &&
                     ((uintptr_t)C.sigma & 15u) == 0;
    const size_t lds = (size_t)((max_cells + 63u) / 64u) * 64u * 4u;
    hipLaunchKernelGGL(k_compact_small, dim3((unsigned)X.n), dim3(kCsBlock), lds, st, X, C, cls, Bm, mw, wide);
    return hipGetLastError();
}

}  // namespace pvhip
