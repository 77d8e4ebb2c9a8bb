// rt_text.cpp — text packing (reference utils/text.hpp:15-37, 63-87) in host memory: 15 message
// bytes per Fp plaintext. No context, no device: builds with a plain host compiler.
#include <stddef.h>
#include <stdint.h>

#include "../../include/pvac_hip.h"

namespace {
// fp_from_words (core/field.hpp:26-48) folds bit 127 back in and maps p to 0. A block's 15 bytes
// fill 120 bits, so hi < 2^56 here and the words pass through unchanged; only the p check is kept.
void fp_words(uint64_t& lo, uint64_t& hi) {
    if (lo == ~0ull && hi == 0x7FFFFFFFFFFFFFFFull) lo = hi = 0;
}
}  // namespace

extern "C" {

int pvac_text_pack(const uint8_t* msg, size_t len, uint64_t* v_out, size_t block_cap, size_t* blocks) {
    if ((len && !msg) || !blocks) return PVAC_EINVAL;
    const size_t nb = len / 15 + (len % 15 ? 1 : 0);
    *blocks = nb;
    if (nb > block_cap) return PVAC_ENOMEM;
    if (nb && !v_out) return PVAC_EINVAL;
    for (size_t b = 0; b < nb; ++b) {
        const size_t pos = b * 15, take = len - pos < 15 ? len - pos : 15;
        uint64_t lo = 0, hi = 0;
        for (size_t i = 0; i < take; ++i) {
            const uint64_t x = msg[pos + i];
            if (i < 8) lo |= x << (8 * i);
            else hi |= x << (8 * (i - 8));
        }
        fp_words(lo, hi);
        v_out[2 * b] = lo;
        v_out[2 * b + 1] = hi;
    }
    return PVAC_OK;
}

int pvac_text_unpack(const uint64_t* dec, size_t n_ciphers, uint8_t* out, size_t cap, size_t* len, uint32_t* flags) {
    if ((n_ciphers && !dec) || !len) return PVAC_EINVAL;
    uint32_t fl = 0;
    uint64_t n = 0;
    if (n_ciphers) {
        n = dec[0];
        if (dec[1] != 0) fl |= PVAC_TEXT_LEN_HI;
        const uint64_t have = 15ull * (uint64_t)(n_ciphers - 1);
        if (have < n) {
            n = have;
            fl |= PVAC_TEXT_LEN_CLIPPED;
        }
    }
    if (flags) *flags = fl;
    *len = (size_t)n;
    if (n > cap) return PVAC_ENOMEM;
    if (n && !out) return PVAC_EINVAL;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t b = 1 + i / 15, j = i % 15;
        out[i] = j < 8 ? (uint8_t)(dec[2 * b] >> (8 * j)) : (uint8_t)(dec[2 * b + 1] >> (8 * (j - 8)));
    }
    return PVAC_OK;
}

}  // extern "C"
