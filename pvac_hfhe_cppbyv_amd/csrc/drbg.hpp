// drbg.hpp — the library's random generator: SP 800-90A rev. 1 §10.2.1 CTR_DRBG with AES-256, no
// derivation function, no prediction resistance, seedlen = 48 bytes (keylen 32 + blocklen 16). Host
// code only, no HIP call: the state lives on the host, and a request for device words is split into
// "this keystream (K, V + 1, nb blocks) goes to the kernel" and "the state advances", so one class
// serves the runtime (k_drbg.hip writes the keystream) and a CPU check (aes_ctr_keystream below).
//
// State: K (32 bytes), V (one 128-bit block, read big-endian; every addition is mod 2^128).
//   update(data[48]):      temp = AES_K(V+1) || AES_K(V+2) || AES_K(V+3); temp ^= data;
//                          K = temp[0..32), V = temp[32..48)
//   instantiate(e[48]):    K = 0, V = 0, update(e)
//   reseed(e[48]):         update(e); the call counter returns to 0
//   generate(n words):     nb = ceil(n / 2); block j (1..nb) = AES_K(V + j); word 2(j-1) = load_le64 of
//                          its bytes 0..7, word 2(j-1)+1 of its bytes 8..15 (csprng_u64 over the
//                          concatenated block bytes; an odd n drops the last 8 bytes); then V += nb,
//                          update(0^48), and the call counter goes up by one. n = 0 is a no-op: the
//                          state is unchanged and the call is not counted.
// One stated deviation from 90A: the cap of 2^16 bytes per request (max_number_of_bits_per_request)
// is lifted, so a call generates what its consumer needs in one kernel launch (a batch of 2^20
// fresh pairs takes 2^26 bytes of nonces). Every other limit holds trivially: a request of 2^64
// words is far below the 2^128 blocks a key may encrypt.
// Seeding: an instance that was given no seed seeds itself with 48 bytes from the entropy source (by
// default getrandom(2)) at its first use, and reseeds from the source once `reseed_interval`
// generate calls (default 2^16) have run since the last (re)seed: generate call interval + 1 reseeds
// first. An explicitly seeded instance never reseeds on its own, which makes tests and replays exact;
// reseed() on it is still the caller's to make.
// Wiping: K, V and every temporary that held key material (the update block, expanded round keys,
// a request's aes_ctr_job once the caller is done with it: wipe()) go through explicit_bzero on
// every key change and on destruction. What is not wiped: the words handed out.
#pragma once
#include <errno.h>
#include <string.h>
#include <sys/random.h>

#include <functional>
#include <mutex>

#include "../../include/pvac_hip.h"
#include "aes256.hpp"

namespace pvhip {

constexpr size_t kDrbgSeedLen = 48;
constexpr uint64_t kDrbgReseedInterval = 1ull << 16;

inline void wipe(void* p, size_t n) { explicit_bzero(p, n); }

inline const aes_ttables& aes_host_tables() {
    static const aes_ttables t = aes_make_tables();
    return t;
}

inline void aes256_host_expand(const uint8_t key[32], uint32_t rk[60]) {
    uint32_t k[8];
    memcpy(k, key, 32);   // little-endian column words
    aes256_expand(k, rk, [](uint32_t x) { return (uint32_t)kAesSbox[x]; });
    wipe(k, sizeof k);
}

// AES_K of the counter block (hi, lo) read big-endian -> 16 bytes
inline void aes256_host_block(const uint32_t rk[60], uint64_t hi, uint64_t lo, uint8_t out[16]) {
    const aes_ttables& t = aes_host_tables();
    uint32_t w[4] = {__builtin_bswap32((uint32_t)(hi >> 32)), __builtin_bswap32((uint32_t)hi),
                     __builtin_bswap32((uint32_t)(lo >> 32)), __builtin_bswap32((uint32_t)lo)};
    aes256_encrypt(w[0], w[1], w[2], w[3], [&](int k, uint32_t x) { return t.T[k][x]; }, [&](int i) { return rk[i]; });
    memcpy(out, w, 16);
}

// the CPU keystream of a job: out[0, n_words), n_words <= 2 nb
inline void aes_ctr_keystream(const aes_ctr_job& job, uint64_t* out, size_t n_words) {
    for (uint64_t j = 0; 2 * j < n_words; ++j) {
        const uint64_t lo = job.ctr_lo + j, hi = job.ctr_hi + (lo < job.ctr_lo ? 1 : 0);
        uint8_t b[16];
        aes256_host_block(job.rk, hi, lo, b);
        memcpy(&out[2 * j], b, 2 * j + 1 < n_words ? 16 : 8);
    }
}

// 48 bytes of getrandom(2); 0, or PVAC_EDEVICE when the kernel gives none
inline int os_entropy(uint8_t out[kDrbgSeedLen]) {
    size_t got = 0;
    while (got < kDrbgSeedLen) {
        const ssize_t r = getrandom(out + got, kDrbgSeedLen - got, 0);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return PVAC_EDEVICE;
        got += (size_t)r;
    }
    return PVAC_OK;
}

class ctr_drbg {
public:
    using entropy_fn = std::function<int(uint8_t out[kDrbgSeedLen])>;   // 0, or an error code

    explicit ctr_drbg(uint64_t reseed_interval = kDrbgReseedInterval, entropy_fn source = os_entropy)
        : interval_(reseed_interval ? reseed_interval : 1), source_(std::move(source)) {}
    ~ctr_drbg() {
        wipe(K_, sizeof K_);
        wipe(&v_hi_, sizeof v_hi_);
        wipe(&v_lo_, sizeof v_lo_);
    }
    ctr_drbg(const ctr_drbg&) = delete;
    ctr_drbg& operator=(const ctr_drbg&) = delete;

    // instantiate; seed == nullptr: from the entropy source (a self-seeded instance). reseeds: a
    // given seed that came from a self-seeded generator (a chain worker's), so this instance reseeds
    // from the source at the interval like its parent
    int seed(const uint8_t* seed, bool reseeds = false) {
        std::lock_guard<std::mutex> g(mu_);
        const int rc = seed_locked(seed);
        if (!rc && reseeds) self_ = true;
        return rc;
    }

    // entropy == nullptr: from the entropy source. An instance not yet seeded seeds itself first.
    int reseed(const uint8_t* entropy) {
        std::lock_guard<std::mutex> g(mu_);
        if (!seeded_) {
            const int rc = seed_locked(nullptr);
            if (rc) return rc;
        }
        return reseed_locked(entropy);
    }

    // A request of n_words words for the caller to produce: job = the keystream (K, V + 1, nb);
    // the state has advanced when this returns, so two requests never share a counter. n_words = 0:
    // job->nb = 0 and nothing else happens. first_block (nullable): the number of blocks handed out
    // before this request since the instance was seeded. The caller wipes *job when it is done.
    int request(size_t n_words, aes_ctr_job* job, uint64_t* first_block = nullptr) {
        std::lock_guard<std::mutex> g(mu_);
        return request_locked(n_words, job, first_block);
    }

    // n words on the host (the CPU keystream)
    int generate(uint64_t* out, size_t n_words, uint64_t* first_block = nullptr) {
        aes_ctr_job job;
        const int rc = request(n_words, &job, first_block);
        if (!rc) aes_ctr_keystream(job, out, n_words);
        wipe(&job, sizeof job);
        return rc;
    }

    // small host-side requests (a child generator's seed): the first `bytes` bytes of the keystream
    // of one generate call of ceil(bytes / 8) words
    int generate_host(uint8_t* out, size_t bytes, uint64_t* first_block = nullptr) {
        const size_t n = (bytes + 7) / 8;
        aes_ctr_job job;
        const int rc = request(n, &job, first_block);
        if (!rc) {
            uint64_t w[2];
            for (size_t i = 0; i < n; i += 2) {
                aes_ctr_job one = job;
                one.ctr_lo = job.ctr_lo + i / 2;
                one.ctr_hi = job.ctr_hi + (one.ctr_lo < job.ctr_lo ? 1 : 0);
                aes_ctr_keystream(one, w, 2);
                const size_t at = 8 * i;
                memcpy(out + at, w, bytes - at < 16 ? bytes - at : 16);
                wipe(&one, sizeof one);
            }
            wipe(w, sizeof w);
        }
        wipe(&job, sizeof job);
        return rc;
    }

    // out[0] generate calls, [1] keystream blocks handed out, [2] reseeds, all since the instance was
    // seeded; [3] = 1 for a self-seeded instance (0: explicitly seeded, or not yet seeded)
    void counts(uint64_t out[4]) {
        std::lock_guard<std::mutex> g(mu_);
        out[0] = calls_;
        out[1] = blocks_;
        out[2] = reseeds_;
        out[3] = seeded_ && self_ ? 1 : 0;
    }

private:
    int draw(uint8_t e[kDrbgSeedLen]) {
        const int rc = source_ ? source_(e) : PVAC_EDEVICE;
        return rc ? PVAC_EDEVICE : PVAC_OK;
    }

    int seed_locked(const uint8_t* seed) {
        uint8_t e[kDrbgSeedLen];
        if (!seed) {
            const int rc = draw(e);
            if (rc) {
                wipe(e, sizeof e);
                return rc;
            }
        } else {
            memcpy(e, seed, sizeof e);
        }
        wipe(K_, sizeof K_);
        v_hi_ = v_lo_ = 0;
        update(e);
        wipe(e, sizeof e);
        seeded_ = true;
        self_ = seed == nullptr;
        calls_ = blocks_ = reseeds_ = since_ = 0;
        return PVAC_OK;
    }

    int reseed_locked(const uint8_t* entropy) {
        uint8_t e[kDrbgSeedLen];
        if (!entropy) {
            const int rc = draw(e);
            if (rc) {
                wipe(e, sizeof e);
                return rc;
            }
        } else {
            memcpy(e, entropy, sizeof e);
        }
        update(e);
        wipe(e, sizeof e);
        since_ = 0;
        ++reseeds_;
        return PVAC_OK;
    }

    int request_locked(size_t n_words, aes_ctr_job* job, uint64_t* first_block) {
        job->nb = 0;
        if (first_block) *first_block = blocks_;
        if (!n_words) return PVAC_OK;
        if (!seeded_) {
            const int rc = seed_locked(nullptr);
            if (rc) return rc;
            if (first_block) *first_block = 0;
        }
        if (self_ && since_ >= interval_) {
            const int rc = reseed_locked(nullptr);
            if (rc) return rc;
        }
        const uint64_t nb = (uint64_t)n_words / 2 + (n_words & 1);
        aes256_host_expand(K_, job->rk);
        job->ctr_lo = v_lo_ + 1;
        job->ctr_hi = v_hi_ + (job->ctr_lo == 0 ? 1 : 0);
        job->nb = nb;
        add_v(nb);
        const uint8_t zero[kDrbgSeedLen] = {0};
        update(zero);
        ++calls_;
        ++since_;
        blocks_ += nb;
        return PVAC_OK;
    }

    void add_v(uint64_t k) {
        const uint64_t lo = v_lo_ + k;
        v_hi_ += lo < v_lo_ ? 1 : 0;
        v_lo_ = lo;
    }

    void update(const uint8_t data[kDrbgSeedLen]) {
        uint32_t rk[60];
        uint8_t temp[kDrbgSeedLen];
        aes256_host_expand(K_, rk);
        for (int j = 0; j < 3; ++j) {
            add_v(1);
            aes256_host_block(rk, v_hi_, v_lo_, temp + 16 * j);
        }
        for (size_t i = 0; i < kDrbgSeedLen; ++i) temp[i] ^= data[i];
        memcpy(K_, temp, 32);
        v_hi_ = v_lo_ = 0;
        for (int i = 0; i < 8; ++i) {   // V = temp[32..48), big-endian
            v_hi_ = (v_hi_ << 8) | temp[32 + i];
            v_lo_ = (v_lo_ << 8) | temp[40 + i];
        }
        wipe(rk, sizeof rk);
        wipe(temp, sizeof temp);
    }

    std::mutex mu_;
    uint8_t K_[32] = {0};
    uint64_t v_hi_ = 0, v_lo_ = 0;
    bool seeded_ = false, self_ = false;
    uint64_t interval_;
    entropy_fn source_;
    uint64_t calls_ = 0, blocks_ = 0, reseeds_ = 0, since_ = 0;
};

}  // namespace pvhip
