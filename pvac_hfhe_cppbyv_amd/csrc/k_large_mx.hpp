// k_large_mx.hpp — the matrix-core pieces shared by the products kernels of the general ct_mul path
// (k_large_products.hip: k_large_products / _la / _defer; k_large_direct.hip: k_large_count_la,
// k_large_products_direct); included only by them.
#pragma once
#include "k_large.hpp"

#include <type_traits>

namespace pvhip {

namespace {

// ---- dense mode on the matrix cores (gfx950 v_mfma_i32_32x32x32_i8) --------------------------
// An Fp value v (canonical) is taken as the signed integer V = v (v < 2^126) or v - p, written
// with 16 balanced base-256 digits d_i in [-128, 127] (int8). For output index r of a task,
//     sum_e D[r - idx_e] * w_e  =  sum_m 256^m  sum_e sum_j W_e[m][j] D[r - idx_e][j],
// W_e[m][j] = digit (m - j) of w_e (zero outside 0..15): a 32 x 32 (digit position m) x (row r)
// tile over K = 2 sparse edges x 16 digits is ONE v_mfma_i32_32x32x32_i8. Column sums stay
// below 2^23 (<= 20 edges x 16 digit pairs x 2^14), so nothing overflows before the epilogue
// turns the 31 digit positions of a row into Fp (mx_fold). Operand maps (tools/mfma_i8_probe.hip):
// A lane l = (m = l & 31, half h = l >> 5) byte j  x  B lane (r = l & 31, h) byte j, for the same
// (h, j); D lane l register i = position (i & 3) + 8 (i >> 2) + 4 h of row l & 31.
typedef int mx_v4 __attribute__((ext_vector_type(4)));
typedef int mx_v16 __attribute__((ext_vector_type(16)));
static_assert(kMxMaxSparse == kIblkMaxSparse, "iblk pairs need every B layer on the matrix cores");
constexpr uint64_t kDigC = 0x8080808080808080ull;  // 128 in every byte

// balanced digits of a canonical value: U = V + C (C = 128 in each of the 16 bytes), d = U ^ C
__device__ __forceinline__ void fp_digits8(const fp& v, uint64_t& dl, uint64_t& dh) {
    const bool neg = (v.hi >> 62) != 0;            // v >= 2^126: V = v - p = v + 2^127 + 1 (mod 2^128)
    const uint64_t l = v.lo + (neg ? 1ull : 0ull);
    const uint64_t h = v.hi + (neg ? 0x8000000000000000ull + (l < v.lo ? 1ull : 0ull) : 0ull);
    const uint64_t ul = l + kDigC;
    const uint64_t uh = h + kDigC + (ul < l ? 1ull : 0ull);
    dl = ul ^ kDigC;
    dh = uh ^ kDigC;
}

// A lane's 16 column sums c[i] sit at digit positions k(i) = (i & 3) + 8 (i >> 2) + 4 h, and
// k(i + 8) = k(i) + 16: 256^16 = 2^128 == 2 (mod p), so d[i] = c[i] + 2 c[i + 8] (32-bit, |d| < 2^24
// for <= 20 sparse edges) leaves positions 4h..4h+3 (d[0..3]) and 8+4h..11+4h (d[4..7]), i.e. the
// 32-bit words h and 2 + h of the row's value: ga, gb (|g| < 2^48.1).
// acc + (int64) x * m in one v_mad_i64_i32 (sign extension, shift and 64-bit add: the compiler's
// form of a power-of-two multiple is a sign-extending shift plus a 64-bit shift-add per term)
__device__ __forceinline__ int64_t mad_i64_i32(int32_t x, uint32_t m, int64_t acc) {
    int64_t r;
    asm volatile("v_mad_i64_i32 %0, vcc, %1, %2, %3" : "=v"(r) : "v"(x), "s"(m), "v"(acc) : "vcc");
    return r;
}
__device__ __forceinline__ void mx_groups(const mx_v16& c, int64_t& ga, int64_t& gb) {
    int32_t d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = c[i] + 2 * c[i + 8];
    ga = mad_i64_i32(d[3], 16777216u, mad_i64_i32(d[2], 65536u, mad_i64_i32(d[1], 256u, (int64_t)d[0])));
    gb = mad_i64_i32(d[7], 16777216u, mad_i64_i32(d[6], 65536u, mad_i64_i32(d[5], 256u, (int64_t)d[4])));
}

// Z = H0 + H1 2^32 + H2 2^64 + H3 2^96 mod p (|H| < 2^56), canonical. 2^128 == 2, 2^127 == 1 (mod p).
__device__ __forceinline__ fp mx_fold(int64_t a0, int64_t a1, int64_t b0, int64_t b1) {
    // 32-bit words W0..W4 of Z; W4 2^128 == 2 W4 goes into W0
    int64_t t = (int64_t)(uint32_t)a0 + 2 * (b1 >> 32);
    const uint32_t x0 = (uint32_t)t;
    t = (t >> 32) + (a0 >> 32) + (int64_t)(uint32_t)a1;
    const uint32_t x1 = (uint32_t)t;
    t = (t >> 32) + (a1 >> 32) + (int64_t)(uint32_t)b0;
    const uint32_t x2 = (uint32_t)t;
    t = (t >> 32) + (b0 >> 32) + (int64_t)(uint32_t)b1;
    const uint32_t x3 = (uint32_t)t;
    const int64_t k = t >> 32;                     // Z == X + 2 k, X = x3..x0 in [0, 2^128), |k| <= 1
    uint64_t lo = (uint64_t)x0 | (uint64_t)x1 << 32, hi = (uint64_t)x2 | (uint64_t)x3 << 32;
    const int64_t s = (int64_t)(hi >> 63) + 2 * k; // X = Xl + 2^127 Xh
    hi &= kM63;
    // Xl + s, or Xl + (p + s) when s < 0: stays in [0, 2^128)
    const uint64_t alo = s < 0 ? kAll - (uint64_t)(-s) : (uint64_t)s;
    const uint64_t ahi = s < 0 ? kM63 : 0ull;
    lo += alo;
    hi += ahi + (lo < alo ? 1ull : 0ull);
    return fp_from_words(lo, hi);
}

__device__ __forceinline__ int64_t shfl_xor64(int64_t v, int mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), mask);
    return (int64_t)((uint64_t)hi << 32 | lo);
}

// LDS of the MFMA dense mode: dig[2][2B] (16 B of digits per dense slot, stored twice per channel
// like the column mode's tables) | tt[2][2B] (the dense side's share of the first-insert time) |
// dup; then, per sparse side, prec[kMxMaxSparse][3] (48 B per sparse edge: 16 zero bytes, its
// digits reversed, 16 zero bytes: W_e's row m is the 16-byte window at 31 - m) and
// pinf[kMxMaxSparse] (uint4: P and M slot offsets relative to row r, the sparse side's share of t).
// Byte offsets of tt and dup (dig sits at 0; iblk_layer's M1 / M2 reuse it):
__host__ __device__ inline uint32_t mx_tt_off(uint32_t Bm) { return 64u * Bm; }
__host__ __device__ inline uint32_t mx_dup_off(uint32_t Bm) { return mx_tt_off(Bm) + 16u * Bm; }
__host__ __device__ inline uint32_t mx_lds_bytes(uint32_t Bm) { return al16(mx_dup_off(Bm) + 4u); }
// k_large_count_la (no digit tables): M1 / M2 [0, 32 B) | tt [32 B, 48 B) | dup | list length, then
// the B layers' staging at cnt_lds_bytes (6 workgroups per CU where mx_lds_bytes allowed 4)
constexpr uint32_t kCntTtOff = 32u;
__host__ __device__ inline uint32_t cnt_tt_off(uint32_t Bm) { return kCntTtOff * Bm; }
__host__ __device__ inline uint32_t cnt_dup_off(uint32_t Bm) { return cnt_tt_off(Bm) + 16u * Bm; }
__host__ __device__ inline uint32_t cnt_len_off(uint32_t Bm) { return cnt_dup_off(Bm) + 4u; }
__host__ __device__ inline uint32_t cnt_lds_bytes(uint32_t Bm) { return al16(cnt_len_off(Bm) + 4u); }

// a key's record (one per output row and B layer; iblk_layer and cnt_layer_list read them): dense slot
// of its A edge | j << 12 | edge bits << 18 | shared << 20 | 1 << 21 (0: no key)
constexpr uint32_t kRecKey = 1u << 21, kRecShared = 1u << 20;

// a sparse-side edge's weight as the middle row of its prec entry: digit 15 - x at byte x
__device__ __forceinline__ uint4 mx_rev_digits(const edge_rec& x) {
    uint64_t dl, dh;
    fp_digits8(fp_canon(x.lo, x.hi), dl, dh);
    const uint64_t rl = __builtin_bswap64(dh), rh = __builtin_bswap64(dl);
    return make_uint4((uint32_t)rl, (uint32_t)(rl >> 32), (uint32_t)rh, (uint32_t)(rh >> 32));
}
// sparse edge k's prec entry: 16 zero bytes, mid, 16 zero bytes
__device__ __forceinline__ void mx_put_prec(uint4* prec, uint32_t k, const uint4& mid) {
    prec[3u * k] = make_uint4(0, 0, 0, 0);
    prec[3u * k + 1u] = mid;
    prec[3u * k + 2u] = make_uint4(0, 0, 0, 0);
}

// A operand of k-step s for lane (half h, row n): row m = n of W_e, e = 2 s + h: 16 bytes at 31 - n
// of prec[e]
template <int NKS>
__device__ __forceinline__ void mx_load_frags(const uint4* prec, uint32_t h, uint32_t n, mx_v4 (&frag)[NKS]) {
    const uint32_t y0 = 31u - n, sh = y0 & 3u;
    const uint32_t* pw = (const uint32_t*)prec + (y0 >> 2) + 12u * h;
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
        const uint32_t* q = pw + 24u * (uint32_t)s;
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4];
        frag[s] = mx_v4{(int)__builtin_amdgcn_alignbyte(w1, w0, sh), (int)__builtin_amdgcn_alignbyte(w2, w1, sh),
                        (int)__builtin_amdgcn_alignbyte(w3, w2, sh), (int)__builtin_amdgcn_alignbyte(w4, w3, sh)};
    }
}

// f(std::integral_constant<int, K>, a...) for the K = ceil(ns / 2) k-steps of a sparse side of ns edges
// (workgroup-uniform): one instantiation of the row loop per k-step count. Nothing for ns = 0.
// dir_rows hands its arguments through a... to a lambda without captures: captured, they pass through
// a closure object, and k_large_products_direct's table addresses are then computed differently (three
// v_lshl_add per k-step for three shifts and two v_add3), which is not the measured code.
template <class F, class... A>
__device__ __forceinline__ void mx_for_ks(uint32_t ns, F f, A... a) {
    static_assert(kMxKS == 10, "one instantiation per k-step count");
    switch ((ns + 1u) >> 1) {
    case 0: return;
    case 1: f(std::integral_constant<int, 1>{}, a...); return;
    case 2: f(std::integral_constant<int, 2>{}, a...); return;
    case 3: f(std::integral_constant<int, 3>{}, a...); return;
    case 4: f(std::integral_constant<int, 4>{}, a...); return;
    case 5: f(std::integral_constant<int, 5>{}, a...); return;
    case 6: f(std::integral_constant<int, 6>{}, a...); return;
    case 7: f(std::integral_constant<int, 7>{}, a...); return;
    case 8: f(std::integral_constant<int, 8>{}, a...); return;
    case 9: f(std::integral_constant<int, 9>{}, a...); return;
    default: f(std::integral_constant<int, 10>{}, a...); return;
    }
}

}  // namespace

}  // namespace pvhip
