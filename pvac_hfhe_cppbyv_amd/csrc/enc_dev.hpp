// enc_dev.hpp — device pieces of enc_fp_depth (reference ops/encrypt.hpp:162-258) shared by
// k_enc.hip (one noise plan per launch, array-of-struct halves) and k_enc_items.hip (a plan per
// item, ragged structure-of-arrays halves): the draw stream, rand_fp_nonzero, the draw replay of
// one half and its PRF requests. The noise plan (Z2, Z3) is an argument; a HALF is anything with the
// fields of k_enc.hip's enc_half (scalars nlo, nhi, ztag, vlo, vhi, npre, nout; key, salt, rlo, rhi,
// grp, slot indexable by pre-edge). Device code only.
#pragma once
#include "common.hpp"
#include "sha256.hpp"

namespace pvhip {

struct rstream {
    const uint64_t* p;
    uint32_t n, i;
    bool over;
    __device__ uint64_t next() {
        if (i < n) return p[i++];
        over = true;
        return 0;
    }
};

__device__ inline fp rand_fp_nonzero(rstream& rs) {   // core/types.hpp:145-155
    for (;;) {
        const uint64_t lo = rs.next();
        const uint64_t hi = rs.next() & kM63;
        const fp x = fp_from_words(lo, hi);
        if ((x.lo | x.hi) || rs.over) return x;
    }
}

__device__ __forceinline__ fp powg_at(const uint64_t* g, uint32_t i) { return fp{g[2 * i], g[2 * i + 1]}; }

// one enc_fp_depth draw replay (ops/encrypt.hpp:162-258, no PRF / weights)
template <class HALF>
__device__ void plan_half(uint64_t canon, uint32_t B, uint32_t Z2, uint32_t Z3, rstream& rs, const fp& v, HALF& H) {
    H.nlo = rs.next();
    H.nhi = rs.next();
    H.ztag = layer_ztag(canon, H.nlo, H.nhi);   // prg_layer_ztag (crypto/matrix.hpp:254-264)
    H.vlo = v.lo;
    H.vhi = v.hi;
    uint32_t idx[8], ch[8];
    for (int j = 0; j < 8; ++j) {   // pick_unique_idx (encrypt.hpp:130-135), then the sign
        uint32_t x;
        bool dup;
        do {
            x = (uint32_t)(rs.next() % B);
            dup = false;
            for (int q = 0; q < j; ++q) dup |= idx[q] == x;
        } while (dup && !rs.over);
        idx[j] = x;
        ch[j] = (uint32_t)(rs.next() & 1);
    }
    for (int j = 0; j < 7; ++j) {
        const fp r = rand_fp_nonzero(rs);
        H.rlo[j] = r.lo;
        H.rhi[j] = r.hi;
    }
    H.rlo[7] = 0;
    H.rhi[7] = 0;
    for (int j = 0; j < 8; ++j) {   // make_edge draws the salt (encrypt.hpp:150-153)
        H.key[j] = idx[j] | (ch[j] << 16);
        H.salt[j] = rs.next();
    }
    uint32_t np = 8;
    for (uint32_t t = 0; t < Z2; ++t) {   // encrypt.hpp:212-229
        const uint32_t i = (uint32_t)(rs.next() % B);
        uint32_t j;
        do { j = (uint32_t)(rs.next() % B); } while (j == i && !rs.over);
        const uint32_t s1 = (uint32_t)(rs.next() & 1), s2 = s1 ^ 1;
        const fp ri = rand_fp_nonzero(rs);
        H.key[np] = i | (s1 << 16); H.rlo[np] = ri.lo; H.rhi[np] = ri.hi; H.salt[np] = rs.next(); ++np;
        H.key[np] = j | (s2 << 16); H.rlo[np] = 0; H.rhi[np] = 0; H.salt[np] = rs.next(); ++np;
    }
    for (uint32_t t = 0; t < Z3; ++t) {   // encrypt.hpp:231-252
        const uint32_t i = (uint32_t)(rs.next() % B);
        uint32_t j, k;
        do { j = (uint32_t)(rs.next() % B); } while (j == i && !rs.over);
        do { k = (uint32_t)(rs.next() % B); } while ((k == i || k == j) && !rs.over);
        const uint32_t s1 = (uint32_t)(rs.next() & 1), s2 = (uint32_t)(rs.next() & 1), s3 = (uint32_t)(rs.next() & 1);
        const fp fa = rand_fp_nonzero(rs), fb = rand_fp_nonzero(rs);
        H.key[np] = i | (s1 << 16); H.rlo[np] = fa.lo; H.rhi[np] = fa.hi; H.salt[np] = rs.next(); ++np;
        H.key[np] = j | (s2 << 16); H.rlo[np] = fb.lo; H.rhi[np] = fb.hi; H.salt[np] = rs.next(); ++np;
        H.key[np] = k | (s3 << 16); H.rlo[np] = 0; H.rhi[np] = 0; H.salt[np] = rs.next(); ++np;
    }
    H.npre = np;
    // compact_edges (encrypt.hpp:39-71) output order: (layer, idx, P before M) over distinct keys.
    // First occurrences marked in slot[] (reused for the order below), then each pre-edge's group is
    // the number of distinct keys below its own: O(np^2)
    auto sk = [&](uint32_t e) { return (H.key[e] & 0xFFFFu) * 2u + (H.key[e] >> 16); };
    uint32_t ng = 0;
    for (uint32_t e = 0; e < np; ++e) {
        const uint32_t k = sk(e);
        bool first = true;
        for (uint32_t q = 0; q < e; ++q) first &= sk(q) != k;
        H.slot[e] = first ? 1u : 0u;
        ng += first ? 1u : 0u;
    }
    for (uint32_t e = 0; e < np; ++e) {
        const uint32_t k = sk(e);
        uint32_t rank = 0;
        for (uint32_t f = 0; f < np; ++f) rank += (H.slot[f] && sk(f) < k) ? 1u : 0u;
        H.grp[e] = (uint8_t)rank;
    }
    // shuffle_edges (encrypt.hpp:155-160) on the ng compacted entries, in place in slot[]
    for (uint32_t g = 0; g < ng; ++g) H.slot[g] = (uint8_t)g;
    for (uint32_t i = ng > 1 ? ng - 1 : 0; i > 0; --i) {
        const uint32_t j = (uint32_t)(rs.next() % (uint64_t)(i + 1));
        const uint8_t t = H.slot[i];
        H.slot[i] = H.slot[j];
        H.slot[j] = t;
    }
    H.nout = ng;
}

// prf requests of one half: prf_R's three cores (seed = the layer seed) and, for every group but
// the last, prf_noise_delta's three cores on the derived seed (encrypt.hpp:113-128, 205-210)
template <class HALF>
__device__ void half_requests(uint32_t Z2, uint32_t Z3, const HALF& H, prf_request* req) {
    for (uint32_t c = 0; c < 3; ++c) req[c] = prf_request{H.ztag, H.nlo, H.nhi, c, 0};
    const uint32_t G = Z2 + Z3;
    for (uint32_t g = 0; g + 1 < G; ++g) {
        const uint64_t gg = (uint64_t)g + 1, kk = (uint64_t)(g < Z2 ? 0 : 1) + 1;
        uint64_t lo = H.nlo ^ (0x9e3779b97f4a7c15ull * gg), hi = H.nhi ^ (0x94d049bb133111ebull * gg);
        uint64_t z = H.ztag ^ (0x517cc1b727220a95ull * gg);
        lo ^= kk;
        hi ^= kk << 32;
        z ^= kk << 48;
        for (uint32_t c = 0; c < 3; ++c) req[3 + 3 * g + c] = prf_request{z, lo, hi, 3 + c, 0};
    }
}

}  // namespace pvhip
