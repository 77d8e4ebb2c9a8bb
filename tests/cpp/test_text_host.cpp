// test_text_host.cpp — pvac_text_pack / pvac_text_unpack (csrc/rt_text.cpp) as a stand-alone host
// program: built with -fsanitize=address,undefined by the Makefile (exact-size heap buffers, so a byte
// past an end is reported) and run by tests/test_text_host.py. No GPU, no libpvac_hip.so.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "pvac_hip.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(x)                                                          \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(x)) { ++g_fail; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); } \
    } while (0)

// utils/text.hpp:15-26 restated
static void pack_ref(const uint8_t* p, size_t len, uint64_t& lo, uint64_t& hi) {
    lo = hi = 0;
    for (size_t i = 0; i < len && i < 15; ++i) {
        const uint64_t b = p[i];
        const size_t sh = i * 8;
        if (sh < 64) lo |= b << sh;
        else hi |= b << (sh - 64);
    }
}

static void roundtrip(size_t len) {
    std::unique_ptr<uint8_t[]> msg(new uint8_t[len ? len : 1]);
    for (size_t i = 0; i < len; ++i) msg[i] = (uint8_t)(i % 5 == 0 ? 0xFF : (i % 5 == 1 ? 0x00 : 31 * i + 7));
    const size_t nb = (len + 14) / 15;
    size_t blocks = 99;
    std::unique_ptr<uint64_t[]> v(new uint64_t[2 * nb + 2]);   // slot 0 = the length cipher
    v[0] = len;
    v[1] = 0;
    CHECK(pvac_text_pack(msg.get(), len, v.get() + 2, nb, &blocks) == PVAC_OK && blocks == nb);
    for (size_t b = 0; b < nb; ++b) {
        uint64_t lo, hi;
        pack_ref(msg.get() + 15 * b, len - 15 * b, lo, hi);
        CHECK(v[2 + 2 * b] == lo && v[3 + 2 * b] == hi);
    }
    if (nb) {
        size_t need = 0;
        CHECK(pvac_text_pack(msg.get(), len, v.get() + 2, nb - 1, &need) == PVAC_ENOMEM && need == nb);
    }
    std::unique_ptr<uint8_t[]> out(new uint8_t[len ? len : 1]);
    size_t got = 99;
    uint32_t flags = 99;
    CHECK(pvac_text_unpack(v.get(), nb + 1, out.get(), len, &got, &flags) == PVAC_OK && got == len && flags == 0);
    CHECK(std::memcmp(out.get(), msg.get(), len) == 0);
    if (len) {
        CHECK(pvac_text_unpack(v.get(), nb + 1, out.get(), len - 1, &got, &flags) == PVAC_ENOMEM && got == len);
        // the length says more than the blocks hold: clipped to 15 x blocks
        v[0] = 15 * nb + 1;
        std::unique_ptr<uint8_t[]> all(new uint8_t[15 * nb]);
        CHECK(pvac_text_unpack(v.get(), nb + 1, all.get(), 15 * nb, &got, &flags) == PVAC_OK && got == 15 * nb &&
              flags == PVAC_TEXT_LEN_CLIPPED);
        CHECK(std::memcmp(all.get(), msg.get(), len) == 0);
        for (size_t i = len; i < 15 * nb; ++i) CHECK(all[i] == 0);
        // a high length word is flagged and otherwise ignored
        v[0] = len;
        v[1] = 7;
        CHECK(pvac_text_unpack(v.get(), nb + 1, out.get(), len, &got, &flags) == PVAC_OK && got == len &&
              flags == PVAC_TEXT_LEN_HI);
    }
}

int main() {
    for (size_t len : {0, 1, 14, 15, 16, 29, 30, 31, 45, 1845}) roundtrip(len);
    size_t got = 99, blocks = 99;
    uint32_t flags = 99;
    CHECK(pvac_text_unpack(nullptr, 0, nullptr, 0, &got, &flags) == PVAC_OK && got == 0 && flags == 0);
    CHECK(pvac_text_pack(nullptr, 0, nullptr, 0, &blocks) == PVAC_OK && blocks == 0);
    CHECK(pvac_text_pack(nullptr, 3, nullptr, 0, &blocks) == PVAC_EINVAL);
    CHECK(pvac_text_unpack(nullptr, 2, nullptr, 0, &got, &flags) == PVAC_EINVAL);
    const uint64_t only_len[2] = {5, 0};   // a length cipher alone: clipped to nothing
    CHECK(pvac_text_unpack(only_len, 1, nullptr, 0, &got, &flags) == PVAC_OK && got == 0 && flags == PVAC_TEXT_LEN_CLIPPED);
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    if (!g_fail) std::printf("text host checks passed\n");
    return g_fail ? 1 : 0;
}
