// k_drbg.hip — k_aes256_ctr: the raw AES-256 counter-mode keystream of csrc/drbg.hpp's CTR_DRBG (and
// of pvac_hip_aes256_ctr) on CDNA4. Block j (0 <= j < nb) is AES_K(ctr + j mod 2^128), the counter
// block read big-endian; out[2j] is load_le64 of its bytes 0..7 and out[2j + 1] of its bytes 8..15.
//
// Round keys: the 60 words are expanded on the host and arrive by value in the kernel arguments, so
// they are uniform and sit in SGPRs; the key is never written to a device buffer by the library (the
// runtime's kernel-argument buffer holds them for the launch: DESIGN.md).
// Counter: a lane forms ctr + j with a 128-bit add (a carry may cross any byte and the 64-bit
// halves) and byte-swaps the four 32-bit pieces into the little-endian column words of aes256.hpp.
// Rounds: aes_lds.hpp's, as in k_prf.hip: T0 in LDS with one private copy per lane (64 KB, no bank
// conflicts, one v_perm per address), T1..T3 as rotations, kLaneBlocks independent blocks per lane so
// the round chains overlap their LDS latencies. 512 threads and 64 KB make two workgroups per CU,
// four waves per SIMD.
// Grid: persistent, grid-stride over tiles of kDrbgTile = 512 * kLaneBlocks blocks; a wave's lanes
// take consecutive blocks, so a wave stores 1 KB runs. At most kDrbgGridCap workgroups (two per CU of
// a 256-CU device); a request under one tile launches one workgroup.
// Stores: out is only 8-byte aligned. Every block of a launch has the same alignment, so the choice
// is uniform: one 16-byte store per block where out is 16-byte aligned, else two 8-byte stores; the
// last block of an odd request writes its low word only. Nothing is written past out[n_words).
#include <algorithm>

#include "common.hpp"
#include "aes256.hpp"
#include "aes_lds.hpp"

namespace pvhip {
namespace {

constexpr int kDB = 512;          // threads per workgroup
constexpr int kLaneBlocks = 2;    // independent AES blocks per lane and pass

static_assert(kDrbgTile == (uint32_t)kDB * kLaneBlocks, "a tile is one pass of a workgroup");

// T0, a compile-time constant of the code object: nothing to upload, on any device
struct t0_table {
    uint32_t v[256];
};
constexpr t0_table make_t0() {
    t0_table t{};
    for (uint32_t x = 0; x < 256; ++x) t.v[x] = aes_t0(x);
    return t;
}
__constant__ t0_table c_t0 = make_t0();

struct round_keys {
    uint32_t w[60];
};

// NB blocks ctr + first + b * kDB (b < NB) side by side; lo / hi: the two words of each
template <int NB>
__device__ __forceinline__ void ctr128_blocks(const round_keys& rk, uint64_t chi, uint64_t clo, uint64_t first,
                                              const ttab& T, uint64_t* lo, uint64_t* hi) {
    uint32_t w[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const uint64_t j = first + (uint64_t)b * kDB;
        const uint64_t l = clo + j;
        const uint64_t h = chi + (l < clo ? 1ull : 0ull);
        w[b][0] = __builtin_bswap32((uint32_t)(h >> 32)) ^ rk.w[0];
        w[b][1] = __builtin_bswap32((uint32_t)h) ^ rk.w[1];
        w[b][2] = __builtin_bswap32((uint32_t)(l >> 32)) ^ rk.w[2];
        w[b][3] = __builtin_bswap32((uint32_t)l) ^ rk.w[3];
    }
#pragma unroll
    for (int r = 1; r < 14; ++r) {
        const uint32_t k0 = rk.w[4 * r], k1 = rk.w[4 * r + 1], k2 = rk.w[4 * r + 2], k3 = rk.w[4 * r + 3];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const uint32_t n0 = col(T, w[b][0], w[b][1], w[b][2], w[b][3], k0);
            const uint32_t n1 = col(T, w[b][1], w[b][2], w[b][3], w[b][0], k1);
            const uint32_t n2 = col(T, w[b][2], w[b][3], w[b][0], w[b][1], k2);
            const uint32_t n3 = col(T, w[b][3], w[b][0], w[b][1], w[b][2], k3);
            w[b][0] = n0; w[b][1] = n1; w[b][2] = n2; w[b][3] = n3;
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const uint32_t n0 = col_last(T, w[b][0], w[b][1], w[b][2], w[b][3], rk.w[56]);
        const uint32_t n1 = col_last(T, w[b][1], w[b][2], w[b][3], w[b][0], rk.w[57]);
        const uint32_t n2 = col_last(T, w[b][2], w[b][3], w[b][0], w[b][1], rk.w[58]);
        const uint32_t n3 = col_last(T, w[b][3], w[b][0], w[b][1], w[b][2], rk.w[59]);
        lo[b] = ((uint64_t)n1 << 32) | n0;
        hi[b] = ((uint64_t)n3 << 32) | n2;
    }
}

__global__ __launch_bounds__(kDB) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_aes256_ctr(round_keys rk, uint64_t chi, uint64_t clo, uint64_t n_words, uint32_t tiles, uint64_t* out) {
    __shared__ __attribute__((aligned(16))) uint8_t Tb[kTBytes];
    PVHIP_TTAB_FILL(Tb, kDB, c_t0.v);
    __syncthreads();
    const ttab T{Tb, ((uint32_t)threadIdx.x & 63u) << 2};
    const bool wide = (((uintptr_t)out) & 15u) == 0;   // uniform: block j lies at out + 16 j bytes
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t first = (uint64_t)t * kDrbgTile + threadIdx.x;
        uint64_t lo[kLaneBlocks], hi[kLaneBlocks];
        ctr128_blocks<kLaneBlocks>(rk, chi, clo, first, T, lo, hi);
#pragma unroll
        for (int b = 0; b < kLaneBlocks; ++b) {
            const uint64_t j = first + (uint64_t)b * kDB;
            if (2 * j >= n_words) continue;
            uint64_t* p = out + 2 * j;
            if (2 * j + 1 == n_words) {   // the last block of an odd request
                p[0] = lo[b];
            } else if (wide) {
                *(ulonglong2*)p = make_ulonglong2(lo[b], hi[b]);
            } else {
                p[0] = lo[b];
                p[1] = hi[b];
            }
        }
    }
}

}  // namespace

hipError_t launch_aes256_ctr(const aes_ctr_job& job, uint64_t* out, size_t n_words, hipStream_t st) {
    if (!n_words) return hipSuccess;
    if (!out || job.nb < ((uint64_t)n_words + 1) / 2) return hipErrorInvalidValue;
    const uint64_t nb = ((uint64_t)n_words + 1) / 2;
    const uint64_t tiles = (nb + kDrbgTile - 1) / kDrbgTile;
    if (tiles > 0xFFFFFFFFull) return hipErrorInvalidValue;   // 2^42 blocks: beyond any device's memory
    const unsigned grid = (unsigned)std::min<uint64_t>(tiles, kDrbgGridCap);
    round_keys rk;
    for (int i = 0; i < 60; ++i) rk.w[i] = job.rk[i];
    hipLaunchKernelGGL(k_aes256_ctr, dim3(grid), dim3(kDB), 0, st, rk, job.ctr_hi, job.ctr_lo, (uint64_t)n_words,
                       (uint32_t)tiles, out);
    for (int i = 0; i < 60; ++i) ((volatile uint32_t*)rk.w)[i] = 0;
    return hipGetLastError();
}

}  // namespace pvhip
