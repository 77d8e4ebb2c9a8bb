// k_gather.hip — pvac_hip_batch_gather: whole ciphers of several resident batches copied into one dense
// batch (the split and its proofs: gather_tiles.hpp; the host side: rt_gather.cpp).
//
// Plan: one thread per output cipher resolves its pick (or, without picks, its place in the
// concatenation), checks it, and records the source's counts and row offsets in the plan's own arrays;
// the library's scans turn the counts into dense offsets and tile offsets. The destination's index arrays
// are written by a further kernel only when no pick was out of range.
//
// Exec: work is dealt in tiles (at most 16 KiB of edge rows or of layer records of one cipher), numbered
// through the output, so one 345 K-edge cipher spreads over the device and 2^20 small ciphers do not
// cost a workgroup each. A lane group (kGatherLanes lanes: a wave, four tiles in flight per workgroup)
// takes a run of consecutive tiles: one binary search, then the cipher index only moves forward, and
// everything that names the tile is wave-uniform (scalar loads). Edge arrays and sigma rows move 16 bytes
// per lane where gather_split_of / gather_sigma_wide allow, with 8-byte heads and tails, so no store
// lands outside the rows of the cipher being copied. No LDS, no barriers.
#include <algorithm>

#include "common.hpp"
#include "gather_tiles.hpp"

// lanes that copy one tile: 64 (a wave; the kept mapping) or 256 (a workgroup; built as a
// variant for tools/exp_gather.py's comparison)
#ifndef PVAC_GATHER_LANES
#define PVAC_GATHER_LANES 64
#endif

namespace pvhip {

namespace {

constexpr uint32_t kGatherLanes = PVAC_GATHER_LANES;
static_assert(kGatherLanes == 64 || kGatherLanes == kGatherBlock, "a tile is copied by a wave or by a workgroup");
constexpr uint32_t kGatherTilesPerBlock = kGatherBlock / kGatherLanes;

__global__ __launch_bounds__(kGatherBlock) void k_gather_pick(gather_plan_args a) {
    const uint64_t k = (uint64_t)blockIdx.x * kGatherBlock + threadIdx.x;
    if (k >= a.m) return;
    uint64_t j, idx;
    if (!a.pick_idx) {   // concatenation: a.first[n_src] == m, so every k has its source
        j = gather_tile_cipher(a.first, a.n_src, k);
        idx = k - a.first[j];
    } else {
        j = a.pick_src ? a.pick_src[k] : 0u;
        idx = a.pick_idx[k];
    }
    uint64_t L = 0, E = 0, lo = 0, eo = 0;
    if (j >= a.n_src || idx >= a.srcs[j].n) {
        atomicAdd(&a.ctl[3], 1ull);
        j = 0;
    } else {
        const pvac_ct_batch& S = a.srcs[j];
        L = S.l_cnt[idx];
        E = S.e_cnt[idx];
        lo = S.l_off[idx];
        eo = S.e_off[idx];
    }
    a.cL[k] = a.oL[k] = L;
    a.cE[k] = a.oE[k] = E;
    a.toff[k] = gather_tiles(E, L, a.g);
    if (a.toff_s) a.toff_s[k] = gather_tiles(E, L, a.gs);
    a.sL[k] = lo;
    a.sE[k] = eo;
    a.src[k] = (uint32_t)j;
}

// the destination's index arrays, once every pick is known to be in range
__global__ __launch_bounds__(kGatherBlock) void k_gather_index(gather_plan_args a, pvac_ct_batch dst) {
    const uint64_t k = (uint64_t)blockIdx.x * kGatherBlock + threadIdx.x;
    if (k >= a.m || a.ctl[3]) return;
    dst.l_cnt[k] = a.cL[k];
    dst.l_off[k] = a.oL[k];
    dst.e_cnt[k] = a.cE[k];
    dst.e_off[k] = a.oE[k];
}

// A row pointer read from the source table is a generic pointer to the compiler (flat loads); the table
// holds device memory only, so the copies read through global-address-space pointers.
using gsrc8 = const __attribute__((address_space(1))) uint64_t*;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // a 16-byte piece (a plain vector in the host pass too)
using gsrc16 = const __attribute__((address_space(1))) u32x4*;
template <class T>
__device__ __forceinline__ gsrc8 in_global(const T* p) {
    return (gsrc8)(uintptr_t)p;
}

// n 16-byte pieces, four loads in flight per lane
__device__ __forceinline__ void copy16(u32x4* __restrict__ d, gsrc16 s, uint64_t n, uint32_t lane) {
    uint64_t i = lane;
    for (; i + 3 * kGatherLanes < n; i += 4 * kGatherLanes) {
        const u32x4 v0 = s[i], v1 = s[i + kGatherLanes], v2 = s[i + 2 * kGatherLanes], v3 = s[i + 3 * kGatherLanes];
        d[i] = v0;
        d[i + kGatherLanes] = v1;
        d[i + 2 * kGatherLanes] = v2;
        d[i + 3 * kGatherLanes] = v3;
    }
    for (; i < n; i += kGatherLanes) d[i] = s[i];
}

__device__ __forceinline__ void copy8(uint64_t* __restrict__ d, gsrc8 s, uint64_t n, uint32_t lane) {
    uint64_t i = lane;
    for (; i + 3 * kGatherLanes < n; i += 4 * kGatherLanes) {
        const uint64_t v0 = s[i], v1 = s[i + kGatherLanes], v2 = s[i + 2 * kGatherLanes], v3 = s[i + 3 * kGatherLanes];
        d[i] = v0;
        d[i + kGatherLanes] = v1;
        d[i + 2 * kGatherLanes] = v2;
        d[i + 3 * kGatherLanes] = v3;
    }
    for (; i < n; i += kGatherLanes) d[i] = s[i];
}

// n words of an edge array: 16 bytes per lane where the two sides agree in parity
__device__ __forceinline__ void copy_words(uint64_t* __restrict__ d, gsrc8 s, uint64_t n, uint32_t lane) {
    const gather_split sp = gather_split_of((uint64_t)(uintptr_t)s >> 3, (uint64_t)(uintptr_t)d >> 3, n);
    if (!sp.pairs) {
        copy8(d, s, n, lane);
        return;
    }
    if (sp.head && lane == 0) d[0] = s[0];
    copy16((u32x4*)(d + sp.head), (gsrc16)(s + sp.head), sp.pairs, lane);
    if (sp.tail && lane == kGatherLanes - 1) d[n - 1] = s[n - 1];
}

template <bool WIDE>
__global__ __launch_bounds__(kGatherBlock) void k_gather_rows(gather_exec_args a) {
    const uint32_t lane = threadIdx.x % kGatherLanes;
    // the group index through a scalar register: all that follows from it stays wave-uniform
    const uint32_t grp = __builtin_amdgcn_readfirstlane(threadIdx.x / kGatherLanes);
    const uint64_t groups = (uint64_t)gridDim.x * kGatherTilesPerBlock;
    uint64_t t, t1;
    gather_run(a.ntiles, groups, (uint64_t)blockIdx.x * kGatherTilesPerBlock + grp, t, t1);
    if (t >= t1) return;
    uint64_t k = gather_tile_cipher(a.toff, a.m, t);
    for (; t < t1; ++t) {
        while (k + 1 < a.m && a.toff[k + 1] <= t) ++k;
        const uint64_t E = a.cE[k], L = a.cL[k];
        const gather_piece p = gather_piece_of(E, L, a.g, t - a.toff[k]);
        const pvac_ct_batch& S = a.srcs[a.src[k]];
        if (p.layers) {
            static_assert(sizeof(pvac_layer) == kGatherLayerBytes, "layer record = 5 u64");
            copy8((uint64_t*)(a.dst.layers + a.oL[k] + p.first), in_global(S.layers + a.sL[k] + p.first), 5 * p.count, lane);
            continue;
        }
        const uint64_t so = a.sE[k] + p.first, dn = a.oE[k] + p.first;
        copy_words(a.dst.meta + dn, in_global(S.meta) + so, p.count, lane);
        copy_words(a.dst.w_lo + dn, in_global(S.w_lo) + so, p.count, lane);
        copy_words(a.dst.w_hi + dn, in_global(S.w_hi) + so, p.count, lane);
        if (a.dst.sigma) {
            const uint64_t sw = a.dst.sigma_words;
            gsrc8 ss = in_global(S.sigma) + so * sw;
            uint64_t* ds = a.dst.sigma + dn * sw;
            if (WIDE) copy16((u32x4*)ds, (gsrc16)ss, p.count * (sw / 2), lane);
            else copy8(ds, ss, p.count * sw, lane);
        }
    }
}

unsigned grid_for(uint64_t items) { return (unsigned)((items + kGatherBlock - 1) / kGatherBlock); }

}  // namespace

hipError_t launch_gather_plan(const gather_plan_args& a, const pvac_ct_batch& dst, uint64_t* scan_scratch, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.ctl, 0, kGatherCtlWords * 8, st);
    if (e != hipSuccess || !a.m) return e;
    hipLaunchKernelGGL(k_gather_pick, dim3(grid_for(a.m)), dim3(kGatherBlock), 0, st, a);
    e = launch_exclusive_scan2_u64(a.oL, a.oE, a.m, scan_scratch, &a.ctl[0], &a.ctl[1], st);
    if (e == hipSuccess) e = launch_exclusive_scan_u64(a.toff, a.m, scan_scratch, &a.ctl[2], st);
    if (e == hipSuccess && a.toff_s) e = launch_exclusive_scan_u64(a.toff_s, a.m, scan_scratch, &a.ctl[4], st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gather_index, dim3(grid_for(a.m)), dim3(kGatherBlock), 0, st, a, dst);
    return hipGetLastError();
}

hipError_t launch_gather_rows(const gather_exec_args& a, bool wide, int num_cus, hipStream_t st) {
    if (!a.ntiles) return hipSuccess;
    const unsigned grid = (unsigned)gather_grid(a.ntiles, kGatherTilesPerBlock, (uint32_t)num_cus);
    if (wide) hipLaunchKernelGGL(k_gather_rows<true>, dim3(grid), dim3(kGatherBlock), 0, st, a);
    else hipLaunchKernelGGL(k_gather_rows<false>, dim3(grid), dim3(kGatherBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace pvhip
