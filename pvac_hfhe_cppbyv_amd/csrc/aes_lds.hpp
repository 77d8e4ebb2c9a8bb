// aes_lds.hpp — the AES-256 round on an LDS T-table, shared by the kernels that run AES on the device
// (k_prf.hip: the LPN PRF's keystream; k_drbg.hip: the CTR_DRBG keystream). Device code only.
//
// T0 with one private copy per lane: entry x of copy c at LDS byte (x << 8) | (c << 2) (64 copies of
// 1 KB), so no two lanes of a lookup share a bank, and a lookup's address is one v_perm of the state
// word: byte k of w into address byte 1, the lane's copy offset (lane * 4) in byte 0. T1..T3 are
// byte rotations of T0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pvhip {

constexpr uint32_t kTBytes = 256u * 256u;

struct ttab {
    const uint8_t* b;   // LDS table
    uint32_t c4;        // lane * 4
    __device__ __forceinline__ uint32_t at(uint32_t addr) const { return *(const uint32_t*)(b + addr); }
    // T0[byte k of w]
    __device__ __forceinline__ uint32_t t0(uint32_t w, uint32_t k) const {
        return at(__builtin_amdgcn_perm(w, c4, 0x0C0C0000u | ((4u + k) << 8)));
    }
    __device__ __forceinline__ uint32_t sbox(uint32_t x) const { return (at((x << 8) | c4) >> 8) & 0xFFu; }
};

// The table fill of a workgroup of `threads` threads from the 256 entries t0 of T0: word i holds
// entry i >> 6; the caller's barrier follows. A macro, not a function: k_prf.hip's device assembly
// stays byte-identical only while the loop stands in the kernel's own body (an inlined helper
// schedules two moves differently).
#define PVHIP_TTAB_FILL(Tb, threads, t0) \
    for (int i = threadIdx.x; i < (int)(kTBytes / 4); i += (threads)) ((uint32_t*)(Tb))[i] = (t0)[i >> 6]

__device__ __forceinline__ uint32_t rotl(uint32_t v, int s) { return __builtin_amdgcn_alignbit(v, v, 32 - s); }

// one AES-256 round column: T0[w0.b0] ^ T1[w1.b1] ^ T2[w2.b2] ^ T3[w3.b3] ^ key (aes256_encrypt's order)
__device__ __forceinline__ uint32_t col(const ttab& T, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t key) {
    return T.t0(w0, 0) ^ rotl(T.t0(w1, 1), 8) ^ rotl(T.t0(w2, 2), 16) ^ rotl(T.t0(w3, 3), 24) ^ key;
}
// last-round column: the S-box bytes (byte 1 of T0) of w0.b0, w1.b1, w2.b2, w3.b3, packed by v_perm
__device__ __forceinline__ uint32_t col_last(const ttab& T, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3,
                                             uint32_t key) {
    const uint32_t v0 = T.t0(w0, 0), v1 = T.t0(w1, 1), v2 = T.t0(w2, 2), v3 = T.t0(w3, 3);
    const uint32_t lo = __builtin_amdgcn_perm(v1, v0, 0x0C0C0501u);   // [v0.b1, v1.b1, 0, 0]
    const uint32_t hi = __builtin_amdgcn_perm(v3, v2, 0x0C0C0501u);   // [v2.b1, v3.b1, 0, 0]
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u) ^ key;          // [lo.b0, lo.b1, hi.b0, hi.b1]
}

}  // namespace pvhip
