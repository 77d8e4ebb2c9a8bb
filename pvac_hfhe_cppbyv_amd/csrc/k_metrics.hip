// k_metrics.hip — per-cipher metrics computed where the ciphers are (reference utils/metrics.hpp):
//   k_sigma_bytehist  the 256 byte counts sigma_shannon (metrics.hpp:43-68) is a function of
//   k_layer_gsum      agg_layer_gsum (metrics.hpp:70-86) of every layer of every cipher
#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "metrics_split.hpp"

namespace pvhip {
namespace {

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------- sigma_bytehist
// Workgroup blockIdx.x serves share blockIdx.x % splits of cipher blockIdx.x / splits
// (metrics_split.hpp: sigma_popcount's split and its two load paths, 16-byte non-temporal loads over a
// dense aligned range, 8-byte loads over rows of mw used words at a stride of sigma_words).
//
// Counters. One shared 256-bin table would serialise: 64 lanes hitting one bin (an all-zero sigma, a
// real input) cost 32 LDS cycles per half wave. Here every bin has kHistCopies = 32 u32 copies,
// tab[bin][lane % 32], so within a ds_add_u32's 32-lane group lane l is alone on bank l whatever the
// bytes are: no conflict for any content, and lanes l and l + 32 (the same word when their bytes are
// equal) are in different groups, where the LDS serialises the two adds. 32 KiB per workgroup.
// Bound. A counter is shared by the 8 threads of one lane residue. Between two folds lies one round of
// the loop below: kHistRoundItems = 256 x 4096 items of the share, so at most 4096 per thread, each
// adding at most 16 bytes: 8 x 4096 x 16 = 2^19 = hist_counter_bound(), far below 2^32, whatever the
// share's size. After every round thread t folds bin t's 32 copies into a 64-bit register and, when
// another round follows, clears them. The rounds of a share are counted from its size, which is the
// same for every thread of the workgroup, so the barriers are uniform. The flush is one u64 per bin
// and share: a plain store when the workgroup owns the whole cipher (splits == 1: all 256 bins, zeros
// included, no memset needed), else one atomic add per non-zero bin into the zeroed hist.
__device__ __forceinline__ void hist_add4(uint32_t* col, uint32_t w) {
    __hip_atomic_fetch_add(col + ((w & 0xFFu) << 5), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(col + (((w >> 8) & 0xFFu) << 5), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(col + (((w >> 16) & 0xFFu) << 5), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(col + ((w >> 24) << 5), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void hist_add8(uint32_t* col, unsigned long long v) {
    hist_add4(col, (uint32_t)v);
    hist_add4(col, (uint32_t)(v >> 32));
}

__global__ __launch_bounds__(kHistBlock) void k_sigma_bytehist(pvac_ct_batch X, uint32_t mw, uint32_t splits, int wide,
                                                               unsigned long long* hist) {
    __shared__ uint32_t tab[256 * kHistCopies];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = blockIdx.x / splits;
    const uint32_t s = blockIdx.x % splits;
    const uint64_t ne = X.e_cnt[i];
    const uint32_t sw = X.sigma_words;
    const uint64_t* base = X.sigma + X.e_off[i] * sw;
    uint64_t ulo, uhi;
    hist_share(hist_units(ne, mw, wide != 0), splits, s, ulo, uhi);
    const uint64_t items = hist_items(uhi - ulo, mw, wide != 0);
    const uint64_t rounds = hist_rounds(items);
    for (uint32_t t = tid; t < 256 * kHistCopies; t += kHistBlock) tab[t] = 0;
    __syncthreads();
    uint32_t* col = tab + (tid & (kHistCopies - 1));
    unsigned long long mine = 0;   // bin tid of this share
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t a = r * kHistRoundItems, b = min(items, a + kHistRoundItems);
        if (wide) {
            const u64x2* p = (const u64x2*)base + ulo;
            uint64_t u = a + tid;
            for (; u + 3 * kHistBlock < b; u += 4 * kHistBlock) {   // four loads in flight per lane
                const u64x2 v0 = __builtin_nontemporal_load(p + u);
                const u64x2 v1 = __builtin_nontemporal_load(p + u + kHistBlock);
                const u64x2 v2 = __builtin_nontemporal_load(p + u + 2 * kHistBlock);
                const u64x2 v3 = __builtin_nontemporal_load(p + u + 3 * kHistBlock);
                hist_add8(col, v0.x);
                hist_add8(col, v0.y);
                hist_add8(col, v1.x);
                hist_add8(col, v1.y);
                hist_add8(col, v2.x);
                hist_add8(col, v2.y);
                hist_add8(col, v3.x);
                hist_add8(col, v3.y);
            }
            for (; u < b; u += kHistBlock) {
                const u64x2 v = __builtin_nontemporal_load(p + u);
                hist_add8(col, v.x);
                hist_add8(col, v.y);
            }
        } else {
            for (uint64_t t = a + tid; t < b; t += kHistBlock) {
                const uint64_t row = t / mw;
                hist_add8(col, base[(ulo + row) * sw + (t - row * mw)]);
            }
        }
        __syncthreads();
        // bin tid: copies read in the order (c + tid) % 32, so the 32 lanes of a group are on 32 banks
        uint32_t* mybin = tab + tid * kHistCopies;
        uint32_t sum = 0;   // <= 256 threads x 4096 x 16 bytes = 2^24 per round
        const bool more = r + 1 < rounds;   // the last round leaves its counters: nothing reads them again
#pragma unroll 8
        for (uint32_t c = 0; c < kHistCopies; ++c) {
            const uint32_t k = (c + tid) & (kHistCopies - 1);
            sum += mybin[k];
            if (more) mybin[k] = 0;
        }
        mine += sum;
        if (more) __syncthreads();
    }
    unsigned long long* out = hist + 256 * i + tid;
    if (splits == 1)
        *out = mine;
    else if (mine)
        atomicAdd(out, mine);
}

// ---------------------------------------------------------------- layer_gsum
// gsum(X, l) = sum over X's edges of layer l of +/- fp_mul(w, powg_B[idx]) (+ for SGN_P), the
// contract of k_check.hip and tests/gsum_model.py: every term is the bit-exact fp_mul, split into
// 43/42/42-bit limbs (fp_split3) and summed per (layer, channel) in u64 with atomics; fewer than 2^21
// terms cannot pass 2^64, and fp_fold3 / fp_sub give the exact residue of P - M.
//
// Persistent workgroups over tiles of four consecutive ciphers. Routes (gsum_route, the same
// function in the size pass that counts them):
//   wave       at most kGsWaveLayers layers and kGsWaveEdges edges: wave w of the workgroup serves
//              cipher 4 tile + w with a 768-byte table of its own, so a fresh-shaped batch (2 layers,
//              40 edges) costs a wave per cipher, not a workgroup
//   workgroup  tables of at most kGsLdsLayers = 3200 layers (dynamic LDS, sized by the launch for the
//              batch's largest such cipher) and fewer than 2^21 edges: all 256 threads
//   large      2^21 edges or more: summed in pieces of kGsPiece = 2^20 edges, each piece folded mod p
//              and fp_add'ed into the output slot (both canonical, so the sum is exact); or more
//              layers than LDS holds: the table lives in a slab of global scratch, taken from a
//              ticket counter by the first large cipher the workgroup meets and kept. Both at once
//              is fine.
// The barriers of the wave phase are executed by all four waves whatever their ciphers are; the
// workgroup phase branches on values every thread loads from the same addresses.
constexpr int kGsBlock = 256;
constexpr uint32_t kGsTile = kGsBlock / 64;
constexpr uint32_t kGsWaveLayers = 16;
constexpr uint32_t kGsWaveEdges = 4096;
constexpr uint32_t kGsLdsLayers = 3200;        // 150 KiB of tables next to 6 KiB of powg and 3 KiB of static tables
constexpr uint32_t kGsPowgLdsBytes = 6144;     // powg_B is staged in LDS while it fits (B <= 384), else read from global
static_assert(kGsLdsLayers * 48u + kGsPowgLdsBytes + 4096u <= 160u * 1024u, "layer_gsum's LDS");
constexpr uint64_t kGsPiece = 1ull << 20;
constexpr uint64_t kGsEdgeLimit = 1ull << 21;

enum : uint32_t { GS_WAVE = 0, GS_WG = 1, GS_LARGE = 2 };
__device__ __forceinline__ uint32_t gsum_route(uint64_t L, uint64_t ne) {
    if (L <= kGsWaveLayers && ne <= kGsWaveEdges) return GS_WAVE;
    return L > kGsLdsLayers || ne >= kGsEdgeLimit ? GS_LARGE : GS_WG;
}

struct gsum_args {
    pvac_ct_batch X;
    const unsigned long long* powg;   // B x (lo, hi)
    uint32_t Bm;
    uint32_t lds_layers;      // layers the launch's dynamic LDS holds; powg follows them when kPgLds
    uint64_t* gsum;
    uint32_t* status;         // nullable
    uint8_t* slabs;           // n_slabs x slab_layers x 48 bytes (null: no cipher needs one)
    uint64_t slab_layers;
    uint64_t n_slabs;
    unsigned long long* ticket;
    uint64_t tiles;
};

// edges [e0, e1) of X into acc[layer][P0 P1 P2 M0 M1 M2], thread t of `stride`; flags idx >= B.
// Acc names the table's address space (LDS: ds_add_u64 at workgroup scope; a global slab: device scope),
// Pg powg's (words lo, hi per entry). Four edges per thread are loaded before the first is summed: the
// loop is a chain of global-load latencies otherwise (one workgroup of a large cipher has a CU to itself).
typedef __attribute__((address_space(3))) unsigned long long lds_u64;
constexpr int kGsBatch = 4;
template <class Acc, int kScope, class Pg>
__device__ __forceinline__ void gs_edges(const pvac_ct_batch& X, uint64_t e0, uint64_t e1, uint32_t L, const Pg* pg,
                                         uint32_t Bm, Acc* acc, uint32_t t, uint32_t stride, uint32_t& bad) {
    for (uint64_t e = e0 + t; e < e1; e += (uint64_t)kGsBatch * stride) {
        uint64_t m[kGsBatch], wl[kGsBatch], wh[kGsBatch];
        bool ok[kGsBatch];
#pragma unroll
        for (int j = 0; j < kGsBatch; ++j) {
            const uint64_t ej = e + (uint64_t)j * stride;
            ok[j] = ej < e1;
            m[j] = ok[j] ? X.meta[ej] : 0;
            wl[j] = ok[j] ? X.w_lo[ej] : 0;
            wh[j] = ok[j] ? X.w_hi[ej] : 0;
        }
#pragma unroll
        for (int j = 0; j < kGsBatch; ++j) {
            if (!ok[j]) continue;
            const uint32_t l = meta_layer(m[j]), idx = meta_idx(m[j]);
            if (idx >= Bm) {
                bad = 2u;
                continue;
            }
            if (l >= L) continue;   // the reference's loop never asks for this layer id
            const fp term = fp_mul(fp{wl[j], wh[j]}, fp{pg[2u * idx], pg[2u * idx + 1u]});
            uint64_t l0, l1, l2;
            fp_split3(term, l0, l1, l2);
            Acc* a = acc + 6u * l + (meta_ch(m[j]) == 0 ? 0u : 3u);
            __hip_atomic_fetch_add(a, (unsigned long long)l0, __ATOMIC_RELAXED, kScope);
            __hip_atomic_fetch_add(a + 1, (unsigned long long)l1, __ATOMIC_RELAXED, kScope);
            __hip_atomic_fetch_add(a + 2, (unsigned long long)l2, __ATOMIC_RELAXED, kScope);
        }
    }
}

__device__ __forceinline__ fp gs_fold(const unsigned long long* a) {
    return fp_sub(fp_fold3(a[0], a[1], a[2]), fp_fold3(a[3], a[4], a[5]));
}

template <bool kPgLds>
__global__ __launch_bounds__(kGsBlock) void k_layer_gsum(gsum_args g) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long gs_dyn[];
    __shared__ unsigned long long wtab[kGsTile][6 * kGsWaveLayers];
    __shared__ uint32_t bad_s, slab_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const pvac_ct_batch& X = g.X;
    typedef typename std::conditional<kPgLds, lds_u64, unsigned long long>::type pg_word;
    const pg_word* pg;
    if constexpr (kPgLds) {
        unsigned long long* stage = gs_dyn + 6u * g.lds_layers;
        for (uint32_t w = tid; w < 2u * g.Bm; w += kGsBlock) stage[w] = g.powg[w];
        __syncthreads();
        pg = (const lds_u64*)stage;
    } else {
        pg = g.powg;
    }
    uint64_t my_slab = ~0ull;
    for (uint64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x) {
        const uint64_t c0 = tile * kGsTile;
        {   // wave phase: cipher c0 + wave when it is small
            const uint64_t ci = c0 + wave;
            const bool live = ci < X.n;
            const uint64_t L = live ? X.l_cnt[ci] : 0, ne = live ? X.e_cnt[ci] : 0;
            const bool small = live && gsum_route(L, ne) == GS_WAVE;
            unsigned long long* acc = wtab[wave];
            if (small)
                for (uint32_t w = lane; w < 6u * (uint32_t)L; w += 64) acc[w] = 0;
            __syncthreads();
            uint32_t b = 0;
            if (small) {
                const uint64_t eo = X.e_off[ci];
                gs_edges<lds_u64, __HIP_MEMORY_SCOPE_WORKGROUP>(X, eo, eo + ne, (uint32_t)L, pg, g.Bm, (lds_u64*)acc, lane, 64, b);
            }
            __syncthreads();
            if (small) {
                b = __ballot(b != 0) ? 2u : 0u;
                if (lane < L) {
                    const fp s = gs_fold(acc + 6u * lane);
                    uint64_t* out = g.gsum + 2 * (X.l_off[ci] + lane);
                    out[0] = s.lo;
                    out[1] = s.hi;
                }
                if (lane == 0 && g.status) g.status[ci] = b;
            }
        }
        for (uint32_t k = 0; k < kGsTile; ++k) {   // workgroup phase: the tile's other ciphers, one at a time
            const uint64_t ci = c0 + k;
            if (ci >= X.n) break;
            const uint64_t L64 = X.l_cnt[ci], ne = X.e_cnt[ci];
            if (gsum_route(L64, ne) == GS_WAVE) continue;
            const bool in_slab = L64 > g.lds_layers;
            if (in_slab && my_slab == ~0ull) {
                if (tid == 0) slab_s = (uint32_t)atomicAdd(g.ticket, 1ull);
                __syncthreads();
                my_slab = slab_s;
            }
            if (in_slab && (!g.slabs || my_slab >= g.n_slabs || L64 > g.slab_layers)) {
                // not reachable with the launch's own size pass: never write past a table
                if (tid == 0 && g.status) g.status[ci] = 0xFFFFFFFFu;
                continue;
            }
            const uint32_t L = (uint32_t)L64;
            unsigned long long* acc = in_slab ? (unsigned long long*)(g.slabs + my_slab * g.slab_layers * 48u) : gs_dyn;
            const uint64_t eo = X.e_off[ci], lo = X.l_off[ci];
            const uint64_t pieces = ne < kGsEdgeLimit ? 1 : (ne + kGsPiece - 1) / kGsPiece;
            if (tid == 0) bad_s = 0;
            for (uint64_t p = 0; p < pieces; ++p) {
                for (uint32_t w = tid; w < 6u * L; w += kGsBlock) acc[w] = 0;
                if (in_slab) __threadfence();   // global slab: each phase's writes / atomics visible to the next
                __syncthreads();
                uint32_t b = 0;
                const uint64_t e0 = eo + (pieces == 1 ? 0 : p * kGsPiece);
                const uint64_t e1 = pieces == 1 ? eo + ne : min(eo + ne, e0 + kGsPiece);
                if (in_slab)
                    gs_edges<unsigned long long, __HIP_MEMORY_SCOPE_AGENT>(X, e0, e1, L, pg, g.Bm, acc, tid, kGsBlock, b);
                else
                    gs_edges<lds_u64, __HIP_MEMORY_SCOPE_WORKGROUP>(X, e0, e1, L, pg, g.Bm, (lds_u64*)gs_dyn, tid, kGsBlock, b);
                if (b) bad_s = b;
                if (in_slab) __threadfence();
                __syncthreads();
                for (uint32_t l = tid; l < L; l += kGsBlock) {   // layer l is this thread's in every piece
                    fp s = gs_fold(acc + 6u * l);
                    uint64_t* out = g.gsum + 2 * (lo + l);
                    if (p) s = fp_add(fp{out[0], out[1]}, s);
                    out[0] = s.lo;
                    out[1] = s.hi;
                }
                __syncthreads();
            }
            if (tid == 0 && g.status) g.status[ci] = bad_s;
            __syncthreads();
        }
    }
}

// The launch's sizes and the route counts in one pass: out[0] = most layers of a workgroup- or
// large-route cipher whose table fits LDS, out[1] = most layers of a cipher that needs a slab,
// out[2..4] = ciphers on the wave / workgroup / large route, out[5] = ciphers that need a slab,
// out[6] = ciphers whose layer count is beyond 2^28 (refused)
__global__ __launch_bounds__(256) void k_gsum_sizes(pvac_ct_batch X, unsigned long long* out) {
    unsigned long long mx_lds = 0, mx_slab = 0, cnt[3] = {0, 0, 0}, n_slab = 0, n_huge = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < X.n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t L = X.l_cnt[i], ne = X.e_cnt[i];
        const uint32_t r = gsum_route(L, ne);
        cnt[r]++;
        if (r == GS_WAVE) continue;
        if (L >> 28) n_huge++;
        else if (L > kGsLdsLayers) {
            mx_slab = max(mx_slab, (unsigned long long)L);
            n_slab++;
        } else {
            mx_lds = max(mx_lds, (unsigned long long)L);
        }
    }
    for (int o = 32; o; o >>= 1) {
        mx_lds = max(mx_lds, (unsigned long long)__shfl_xor(mx_lds, o));
        mx_slab = max(mx_slab, (unsigned long long)__shfl_xor(mx_slab, o));
        cnt[0] += __shfl_xor(cnt[0], o);
        cnt[1] += __shfl_xor(cnt[1], o);
        cnt[2] += __shfl_xor(cnt[2], o);
        n_slab += __shfl_xor(n_slab, o);
        n_huge += __shfl_xor(n_huge, o);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(out, mx_lds);
        atomicMax(out + 1, mx_slab);
        if (cnt[0]) atomicAdd(out + 2, cnt[0]);
        if (cnt[1]) atomicAdd(out + 3, cnt[1]);
        if (cnt[2]) atomicAdd(out + 4, cnt[2]);
        if (n_slab) atomicAdd(out + 5, n_slab);
        if (n_huge) atomicAdd(out + 6, n_huge);
    }
}

}  // namespace

hipError_t launch_sigma_bytehist(const pvac_ct_batch& X, uint32_t m_bits, int num_cus, unsigned long long* hist, int* wide_out,
                                 hipStream_t st) {
    if (!X.n) return hipSuccess;
    const uint32_t mw = (m_bits + 63) / 64;
    const uint32_t splits = hist_splits(X.n, (uint32_t)num_cus);
    const uint64_t grid = hist_grid(X.n, splits);
    if (!grid) return hipErrorInvalidValue;
    const int wide = hist_wide(mw, X.sigma_words, (uint64_t)(uintptr_t)X.sigma) ? 1 : 0;
    if (splits > 1) {
        const hipError_t e = hipMemsetAsync(hist, 0, X.n * 256 * 8, st);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_sigma_bytehist, dim3((unsigned)grid), dim3(kHistBlock), 0, st, X, mw, splits, wide, hist);
    *wide_out = wide;
    return hipGetLastError();
}

hipError_t launch_gsum_sizes(const pvac_ct_batch& X, unsigned long long* out, hipStream_t st) {
    if (!X.n) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<uint64_t>((X.n + 255) / 256, 1024);
    hipLaunchKernelGGL(k_gsum_sizes, dim3(blocks), dim3(256), 0, st, X, out);
    return hipGetLastError();
}

uint64_t gsum_workgroups(uint64_t n, const unsigned long long* sizes, int num_cus) {
    const uint64_t tiles = (n + kGsTile - 1) / kGsTile;
    // residency: the dynamic table and powg next to 4 KiB of static LDS in 160 KiB, at most 8 workgroups per CU
    const uint64_t lds = sizes[0] * 48 + kGsPowgLdsBytes + 4096;
    const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>(8, 160u * 1024u / lds));
    return std::max<uint64_t>(1, std::min<uint64_t>(tiles, per_cu * (uint64_t)num_cus));
}

uint64_t gsum_slab_count(uint64_t n, const unsigned long long* sizes, int num_cus) {
    return std::min<uint64_t>(sizes[5], gsum_workgroups(n, sizes, num_cus));
}

uint64_t gsum_slab_bytes(uint64_t n, const unsigned long long* sizes, int num_cus) {
    return gsum_slab_count(n, sizes, num_cus) * sizes[1] * 48;
}

// sizes: k_gsum_sizes' words on the host; slabs: gsum_slab_bytes of scratch (null when that is 0);
// ticket: one device u64, zeroed here
hipError_t launch_layer_gsum(const pvac_ct_batch& X, const uint64_t* powg, uint32_t Bm, const unsigned long long* sizes,
                             uint64_t* gsum, uint32_t* status, uint8_t* slabs, unsigned long long* ticket, int num_cus,
                             hipStream_t st) {
    if (!X.n) return hipSuccess;
    if (sizes[5] && !slabs) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(ticket, 0, 8, st);
    if (e != hipSuccess) return e;
    gsum_args g{};
    g.X = X;
    g.powg = (const unsigned long long*)powg;
    g.Bm = Bm;
    g.lds_layers = (uint32_t)sizes[0];
    g.gsum = gsum;
    g.status = status;
    g.slabs = slabs;
    g.slab_layers = sizes[1];
    g.n_slabs = gsum_slab_count(X.n, sizes, num_cus);
    g.ticket = ticket;
    g.tiles = (X.n + kGsTile - 1) / kGsTile;
    const uint64_t blocks = gsum_workgroups(X.n, sizes, num_cus);
    if (16ull * Bm <= kGsPowgLdsBytes)
        hipLaunchKernelGGL(k_layer_gsum<true>, dim3((unsigned)blocks), dim3(kGsBlock), (size_t)sizes[0] * 48 + 16ull * Bm, st, g);
    else
        hipLaunchKernelGGL(k_layer_gsum<false>, dim3((unsigned)blocks), dim3(kGsBlock), (size_t)sizes[0] * 48, st, g);
    return hipGetLastError();
}

}  // namespace pvhip
