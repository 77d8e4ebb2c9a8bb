// commit_msg.hpp — the message of commit_ct (ops/commit.hpp:12-88), stated once for host and device.
//
// One SHA-256 per cipher over
//   "pvac.dom.commit" (15 bytes) | H_digest (32) | le64 canon_tag                          55 bytes
//   per layer: u8 rule, then BASE (rule 0): le64 ztag, nonce_lo, nonce_hi                  25 bytes
//                            any other rule: le64 pa, le64 pb (the u32 fields widened)     17 bytes
//   per edge : le64 layer_id, le64 idx, u8 ch, le64 w_lo, le64 (w_hi & 2^63 - 1)           33 bytes
//              then the first sigma_bytes = (m_bits + 7) / 8 bytes of its sigma row (little-endian
//              words, a partial last word, the top bits of the last byte as stored); none when
//              the batch carries no sigma ("weights-only commit")
//   FIPS 180-4 padding.
//
// commit_feeder turns that into 64-byte blocks without ever indexing registers at run time: the
// byte stream is kept as little-endian 32-bit words (a le64 field at a byte offset of 0..3 is two
// funnel shifts), words go through a 32-word ring the caller provides (LDS on the device, an array
// on the host), and a block is 16 ring words byte-swapped on the way out. A feeder produces whole
// pieces (a layer, an edge head, up to 64 sigma bytes, the padding) until 16 words are ready, so
// the compression itself is called from one place, once per block, by every lane that has one.
#pragma once
#include <stdint.h>

#include "../../include/pvac_hip.h"
#include "sha256.hpp"

namespace pvhip {

constexpr uint32_t kCommitHeadWords = 14;   // the 55 fixed bytes: 13 words and a 3-byte carry
constexpr uint32_t kCommitRingWords = 32;   // a power of two; see commit_feeder::step for the bound

// The 55 bytes every cipher's message starts with, as little-endian words (byte 55 is zero).
inline void commit_head_words(const uint8_t H_digest[32], uint64_t canon_tag, uint32_t w[kCommitHeadWords]) {
    uint8_t m[4 * kCommitHeadWords] = {0};
    const char* lab = "pvac.dom.commit";
    for (int i = 0; i < 15; ++i) m[i] = (uint8_t)lab[i];
    for (int i = 0; i < 32; ++i) m[15 + i] = H_digest[i];
    for (int i = 0; i < 8; ++i) m[47 + i] = (uint8_t)(canon_tag >> (8 * i));
    for (uint32_t i = 0; i < kCommitHeadWords; ++i)
        w[i] = (uint32_t)m[4 * i] | (uint32_t)m[4 * i + 1] << 8 | (uint32_t)m[4 * i + 2] << 16 | (uint32_t)m[4 * i + 3] << 24;
}

// One cipher of a batch: row pointers already at its first layer / edge slot.
struct commit_cipher {
    const pvac_layer* layers;
    const uint64_t *meta, *w_lo, *w_hi;
    const uint64_t* sigma;   // the first edge's row; read only when sigma_bytes != 0
    uint64_t nL, nE;
    uint32_t sigma_words;    // row stride in u64
    uint32_t sigma_bytes;    // bytes hashed per row, 0 = weights only
};

PVH_HD commit_cipher commit_cipher_of(const pvac_ct_batch& X, uint64_t i, uint32_t sigma_bytes) {
    commit_cipher c;
    const uint64_t lo = X.l_off[i], eo = X.e_off[i];
    c.nL = X.l_cnt[i];
    c.nE = X.e_cnt[i];
    c.layers = X.layers + lo;
    c.meta = X.meta + eo;
    c.w_lo = X.w_lo + eo;
    c.w_hi = X.w_hi + eo;
    c.sigma = sigma_bytes ? X.sigma + eo * X.sigma_words : nullptr;
    c.sigma_words = X.sigma_words;
    c.sigma_bytes = sigma_bytes;
    return c;
}

// Ring: void put(uint32_t i, uint32_t w), uint32_t get(uint32_t i) for i < kCommitRingWords.
template <class Ring>
struct commit_feeder {
    enum : uint32_t { LAYERS, EDGE, SIGMA, MARK, TAIL, DONE };
    uint32_t phase;
    uint32_t carry, pend;   // the stream's last 0..3 bytes, not yet a word
    uint32_t fill, rd;      // ring words ready, ring read position
    uint32_t sub;           // SIGMA: bytes of the current row already fed
    uint64_t wr;            // words written since begin()
    uint64_t item;          // layer or edge index; from MARK on the message length in bits

    PVH_HD void reset() { phase = DONE; fill = 0; }
    PVH_HD bool ready() const { return fill >= 16; }
    PVH_HD bool idle() const { return phase == DONE && fill == 0; }

    PVH_HD void word(Ring& r, uint32_t w) {
        r.put((uint32_t)wr & (kCommitRingWords - 1), w);
        ++wr;
        ++fill;
    }
    PVH_HD void push8(Ring& r, uint64_t x) {
        const uint32_t sh = 8 * pend;
        const uint64_t lo = (x << sh) | carry;
        word(r, (uint32_t)lo);
        word(r, (uint32_t)(lo >> 32));
        carry = (uint32_t)((x >> 32) >> (32 - sh));   // x >> (64 - sh), defined at sh = 0
    }
    PVH_HD void push1(Ring& r, uint32_t b) {
        carry |= (b & 0xFFu) << (8 * pend);
        if (++pend == 4) {
            word(r, carry);
            carry = 0;
            pend = 0;
        }
    }

    PVH_HD void begin(Ring& r, const uint32_t head[kCommitHeadWords], const commit_cipher& c) {
        wr = 0;
        fill = 0;
        rd = 0;
#pragma unroll
        for (uint32_t i = 0; i + 1 < kCommitHeadWords; ++i) word(r, head[i]);
        carry = head[kCommitHeadWords - 1];
        pend = 3;
        item = 0;
        sub = 0;
        phase = c.nL ? LAYERS : (c.nE ? EDGE : MARK);
    }

    PVH_HD void next_edge(const commit_cipher& c) {
        phase = ++item == c.nE ? MARK : EDGE;
    }

    // One piece. Called with fill < 16; the largest piece is the padding's TAIL (15 zero words and
    // the length, 17 words), so fill never passes 15 + 17 = kCommitRingWords.
    PVH_HD void step(Ring& r, const commit_cipher& c) {
        switch (phase) {
        case LAYERS: {
            const pvac_layer l = c.layers[item];
            push1(r, l.rule);
            if (l.rule == 0) {
                push8(r, l.ztag);
                push8(r, l.nonce_lo);
                push8(r, l.nonce_hi);
            } else {
                push8(r, l.pa);
                push8(r, l.pb);
            }
            if (++item == c.nL) {
                item = 0;
                phase = c.nE ? EDGE : MARK;
            }
            break;
        }
        case EDGE: {
            const uint64_t m = c.meta[item];
            push8(r, (uint32_t)m);
            push8(r, (m >> 32) & 0xFFFFu);
            push1(r, (uint32_t)(m >> 48));
            push8(r, c.w_lo[item]);
            push8(r, c.w_hi[item] & 0x7FFFFFFFFFFFFFFFull);
            if (c.sigma_bytes) {
                phase = SIGMA;
                sub = 0;
            } else {
                next_edge(c);
            }
            break;
        }
        case SIGMA: {
            const uint64_t* row = c.sigma + item * c.sigma_words + (sub >> 3);   // sub is a multiple of 64
            const uint32_t left = c.sigma_bytes - sub;
            if (left >= 64) {
                uint64_t v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = row[k];
#pragma unroll
                for (int k = 0; k < 8; ++k) push8(r, v[k]);
                sub += 64;
            } else {
                const uint32_t full = left >> 3, tail = left & 7;
                for (uint32_t k = 0; k < full; ++k) push8(r, row[k]);
                if (tail) {
                    const uint64_t x = row[full];
                    for (uint32_t b = 0; b < tail; ++b) push1(r, (uint32_t)(x >> (8 * b)));
                }
                sub = c.sigma_bytes;
            }
            if (sub == c.sigma_bytes) next_edge(c);
            break;
        }
        case MARK: {
            item = (4 * wr + pend) * 8;   // the message length in bits, kept for TAIL
            push1(r, 0x80u);
            while (pend) push1(r, 0);
            phase = TAIL;
            break;
        }
        case TAIL: {
            while ((wr & 15) != 14) word(r, 0);
            word(r, bswap32((uint32_t)(item >> 32)));   // big-endian length; take() swaps it back
            word(r, bswap32((uint32_t)item));
            phase = DONE;
            break;
        }
        default:
            break;
        }
    }

    // Pieces until a block is ready or the message has ended (then fill is a multiple of 16).
    PVH_HD void fill_block(Ring& r, const commit_cipher& c) {
        while (fill < 16 && phase != DONE) step(r, c);
    }
    // The next block as the 16 big-endian words sha_compress takes. Needs ready().
    PVH_HD void take(Ring& r, uint32_t blk[16]) {
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) blk[i] = bswap32(r.get((rd + i) & (kCommitRingWords - 1)));
        rd = (rd + 16) & (kCommitRingWords - 1);
        fill -= 16;
    }
};

// The digest bytes of a finished state (big-endian words, FIPS 180-4).
PVH_HD void commit_digest_bytes(const sha_state& st, uint8_t out[32]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        out[4 * i] = (uint8_t)(st.h[i] >> 24);
        out[4 * i + 1] = (uint8_t)(st.h[i] >> 16);
        out[4 * i + 2] = (uint8_t)(st.h[i] >> 8);
        out[4 * i + 3] = (uint8_t)st.h[i];
    }
}

// One cipher start to end on a ring of the caller's: the host route (tests, tools) and the model
// of what each lane of k_commit_ct does between taking a cipher and writing its digest.
template <class Ring>
PVH_HD void commit_one(Ring& r, const uint32_t head[kCommitHeadWords], const commit_cipher& c, uint8_t out[32]) {
    commit_feeder<Ring> f;
    sha_state st;
    sha_init(st);
    f.begin(r, head, c);
    for (;;) {
        f.fill_block(r, c);
        if (!f.ready()) break;
        uint32_t blk[16];
        f.take(r, blk);
        sha_compress(st, blk);
    }
    commit_digest_bytes(st, out);
}

struct commit_host_ring {
    uint32_t w[kCommitRingWords];
    PVH_HD void put(uint32_t i, uint32_t x) { w[i] = x; }
    PVH_HD uint32_t get(uint32_t i) const { return w[i]; }
};

}  // namespace pvhip
