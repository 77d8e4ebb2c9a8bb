// ct_image.hpp — the .ct file image (ct_codec.cpp:3-12) as the device codec sees it, stated once for
// host and device: record geometry, the edge region as a stream of 32-bit words, the layer records
// byte by byte, the layer walks of the two plan passes and the validation of one cipher of an image.
//
// An edge record is eb = 28 + 8 nw bytes, nw = ceil(nbits / 64): a multiple of 4, never of 8. Its first 8
// bytes are meta & (2^56 - 1) (pvac_ct_batch.meta packs the .ct edge header), so a cipher's edge region
// is a stream of wpe = 7 + 2 nw words per edge
//     meta_lo | meta_hi & 0xFFFFFF | w_lo (2) | w_hi (2) | nbits | sigma words, low half first
// shifted by the region's byte offset in the file. Layer records are 9 or 25 bytes, so that offset takes
// every value mod 16: an aligned 16-byte granule of the image is five consecutive stream words funnel-
// shifted by the offset's low two bits. Edge records are uniform and the last cipher's end is the
// file's end, so a cipher's edge region starts at pos[i + 1] - |E| eb without walking its layers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pvac_hip.h"

namespace pvhip {

#ifndef PVH_HD
#define PVH_HD __host__ __device__ __forceinline__
#endif

constexpr uint32_t kCtMagic = 0x66699666u;
constexpr uint32_t kCtVersion = 1u;
constexpr uint32_t kCtFileHdr = 16;      // magic, version, n_ciphers
constexpr uint32_t kCtCipherHdr = 8;     // |L|, |E|
constexpr uint32_t kCtTileBytes = 16384; // an edge tile: whole edge records of at most this many bytes

struct ct_geom {
    uint32_t nbits, nw;   // sigma bits and words per edge on disk
    uint32_t wpe;         // stream words per edge, 7 + 2 nw
    uint32_t ept;         // edges per tile, kCtTileBytes / eb (at least 1)
    PVH_HD uint64_t eb() const { return 4ull * wpe; }
};
PVH_HD ct_geom ct_geom_of(uint32_t nbits) {
    ct_geom g;
    g.nbits = nbits;
    g.nw = nbits / 64u + (nbits % 64u ? 1u : 0u);
    g.wpe = 7u + 2u * g.nw;
    g.ept = kCtTileBytes / (4u * g.wpe);
    if (!g.ept) g.ept = 1;
    return g;
}

// bytes of a layer record: the rule byte, then 8 (PROD) or 24 (BASE and every other rule)
PVH_HD uint32_t ct_layer_bytes(uint32_t rule) { return rule == 1u ? 9u : 25u; }

// byte k of layer y's record (k < ct_layer_bytes(y.rule)); a rule other than 0 or 1 is its byte and zeros
PVH_HD uint8_t ct_layer_byte(const pvac_layer& y, uint32_t k) {
    if (k == 0) return (uint8_t)y.rule;
    k -= 1;
    if (y.rule == 0) {
        const uint64_t w = k < 8 ? y.ztag : k < 16 ? y.nonce_lo : y.nonce_hi;
        return (uint8_t)(w >> (8 * (k & 7)));
    }
    if (y.rule == 1) return (uint8_t)((k < 4 ? y.pa : y.pb) >> (8 * (k & 3)));
    return 0;
}

// The write plan's layer walk: bytes of the layer records of layers [first, first + count) taken with
// `stride` (a lane group shares one cipher); *bad counts the rules >= 256, whose record the host
// writer sizes by the u32 and writes by its low byte.
PVH_HD uint64_t ct_layer_bytes_sum(const pvac_layer* L, uint64_t first, uint64_t count, uint64_t stride, uint32_t* bad) {
    uint64_t b = 0;
    for (uint64_t l = first; l < count; l += stride) {
        const uint32_t rule = L[l].rule;
        if (rule >= 256u) ++*bad;
        b += ct_layer_bytes(rule);
    }
    return b;
}

// The edge rows of one cipher: pointers already at its first edge slot.
struct ct_edge_view {
    const uint64_t *meta, *w_lo, *w_hi;
    const uint64_t* sigma;   // the first edge's row; read only when nw != 0
    uint32_t sigma_words;    // row stride in u64
};
PVH_HD ct_edge_view ct_edge_view_of(const pvac_ct_batch& X, uint64_t i, const ct_geom& g) {
    ct_edge_view v;
    const uint64_t eo = X.e_off[i];
    v.meta = X.meta + eo;
    v.w_lo = X.w_lo + eo;
    v.w_hi = X.w_hi + eo;
    v.sigma = g.nw ? X.sigma + eo * X.sigma_words : nullptr;
    v.sigma_words = X.sigma_words;
    return v;
}

// word k (< wpe) of edge e's record
PVH_HD uint32_t ct_edge_word(const ct_edge_view& v, const ct_geom& g, uint64_t e, uint32_t k) {
    if (k < 2) {
        const uint64_t m = v.meta[e];
        return k ? (uint32_t)(m >> 32) & 0xFFFFFFu : (uint32_t)m;
    }
    if (k < 6) {
        const uint64_t w = k < 4 ? v.w_lo[e] : v.w_hi[e];
        return (uint32_t)(w >> (32 * (k & 1)));
    }
    if (k == 6) return g.nbits;
    const uint64_t s = v.sigma[e * v.sigma_words + ((k - 7) >> 1)];
    return (uint32_t)(s >> (32 * ((k - 7) & 1)));
}

// word j of the cipher's edge stream; words before the stream (j < 0) and past it are 0
PVH_HD uint32_t edge_stream_word(const ct_edge_view& v, const ct_geom& g, uint64_t nE, int64_t j) {
    if (j < 0 || (uint64_t)j >= nE * g.wpe) return 0;
    const uint64_t e = (uint64_t)j / g.wpe;
    return ct_edge_word(v, g, e, (uint32_t)((uint64_t)j - e * g.wpe));
}

// bytes r .. r + 3 of the little-endian pair (lo, hi), r = 0 .. 3
PVH_HD uint32_t ct_funnel(uint32_t lo, uint32_t hi, uint32_t r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, r);
#else
    return r ? (lo >> (8 * r)) | (hi << (32 - 8 * r)) : lo;
#endif
}

// The aligned 16-byte granule of the image at byte address a (a multiple of 16) as four words, for a
// cipher whose edge region starts at byte es: stream bytes a - es .. a - es + 15 (bytes outside the
// region come out as 0; the caller stores only the region's own).
PVH_HD void ct_edge_granule(const ct_edge_view& v, const ct_geom& g, uint64_t nE, uint64_t es, uint64_t a, uint32_t out[4]) {
    const int64_t s = (int64_t)a - (int64_t)es;
    const int64_t j = s >> 2;             // floor: a - es may be -15 .. -1 in a region's first granule
    const uint32_t r = (uint32_t)s & 3u;
    uint32_t w[5];
    for (int k = 0; k < 5; ++k) w[k] = edge_stream_word(v, g, nE, j + k);
    for (int k = 0; k < 4; ++k) out[k] = ct_funnel(w[k], w[k + 1], r);
}

// ---------------------------------------------------------------- reading an image
// The u32 at byte offset off of the image through aligned loads; reads no byte at or past
// (off + 4 + 3) & ~3, which is inside the image's rounded length whenever off + 4 <= len.
PVH_HD uint32_t ct_image_u32(const uint32_t* img32, uint64_t off) {
    const uint64_t a = off >> 2;
    const uint32_t r = (uint32_t)off & 3u;
    const uint32_t lo = img32[a];
    return r ? ct_funnel(lo, img32[a + 1], r) : lo;
}
PVH_HD uint8_t ct_image_u8(const uint32_t* img32, uint64_t off) {
    return (uint8_t)(img32[off >> 2] >> (8 * ((uint32_t)off & 3u)));
}

// The parse plan's layer walk: `count` records from byte `from` must end exactly at byte `to`. Every
// record is at least 9 bytes, so a count the span cannot hold is refused before a byte is read.
PVH_HD bool ct_layer_walk(const uint32_t* img32, uint64_t from, uint64_t to, uint64_t count) {
    if (to < from || count > (to - from) / 9u) return false;
    uint64_t off = from;
    for (uint64_t l = 0; l < count; ++l) {
        if (off >= to) return false;
        off += ct_layer_bytes(ct_image_u8(img32, off));
    }
    return off == to;
}

// Validation of cipher i of an image of len bytes from pos, len and its two count words alone:
// 0 = well-formed (*nL, *nE set), 1 = malformed (*nL = *nE = 0). Reads only bytes inside
// [pos[i], pos[i + 1]), itself checked to lie inside [16, len].
PVH_HD uint32_t ct_parse_validate(const uint32_t* img32, uint64_t len, const uint64_t* pos, uint64_t n, uint64_t i,
                                  const ct_geom& g, uint64_t* nL, uint64_t* nE) {
    *nL = *nE = 0;
    const uint64_t p0 = pos[i], p1 = pos[i + 1];
    if (i == 0 && p0 != kCtFileHdr) return 1;
    if (i + 1 == n && p1 != len) return 1;
    if (p0 < kCtFileHdr || p1 < p0 || p1 > len || p1 - p0 < kCtCipherHdr) return 1;
    const uint64_t L = ct_image_u32(img32, p0), E = ct_image_u32(img32, p0 + 4);
    const uint64_t span = p1 - p0;
    if (E > (span - kCtCipherHdr) / g.eb()) return 1;   // 8 + |E| eb <= span, without the product overflowing
    if (!ct_layer_walk(img32, p0 + kCtCipherHdr, p1 - E * g.eb(), L)) return 1;
    *nL = L;
    *nE = E;
    return 0;
}

}  // namespace pvhip
