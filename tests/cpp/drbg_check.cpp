// drbg_check.cpp — CPU-only checks of csrc/drbg.hpp, the CTR_DRBG class behind pvac_hip_drbg_*: a
// stand-alone host program (tests/cpp/drbg.mk builds it under ASan + UBSan, and once more under TSan;
// tests/test_drbg_host.py runs both).
//   drbg_check <script>   the built-in checks, then the script tests/test_drbg_host.py wrote with
//                         tests/drbg_model.py, one operation per line, every output compared:
//                           seed <96 hex>  |  reseed <96 hex>  |  gen <n> <16 n hex>  (n words on the
//                           CPU keystream; "-" for no output)  |  dev <n> <16 n hex>  (a device-split request: the job's
//                           keystream)  |  host <k> <2 k hex>  (generate_host)  |  counts <c> <b> <r> <s>
//   drbg_check threads    4 threads of generate_host on one instance: no block index is handed out
//                         twice (the TSan build's run)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "drbg.hpp"

using namespace pvhip;

static int g_fail = 0;
#define CHECK(c, ...)                                    \
    do {                                                 \
        if (!(c)) {                                      \
            std::fprintf(stderr, "FAIL %d: ", __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);           \
            std::fprintf(stderr, "\n");                  \
            ++g_fail;                                    \
        }                                                \
    } while (0)

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v(s.size() / 2);
    for (size_t i = 0; i < v.size(); ++i) v[i] = (uint8_t)std::strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return v;
}
static std::string hex(const void* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        s += d[((const uint8_t*)p)[i] >> 4];
        s += d[((const uint8_t*)p)[i] & 15];
    }
    return s;
}

// the raw keystream of (key, ctr) through the class's CPU path
static std::string keystream_hex(const std::string& key_hex, const std::string& ctr_hex, size_t n_words) {
    const std::vector<uint8_t> key = unhex(key_hex), ctr = unhex(ctr_hex);
    aes_ctr_job job;
    aes256_host_expand(key.data(), job.rk);
    job.ctr_hi = job.ctr_lo = 0;
    for (int i = 0; i < 8; ++i) {
        job.ctr_hi = (job.ctr_hi << 8) | ctr[i];
        job.ctr_lo = (job.ctr_lo << 8) | ctr[8 + i];
    }
    job.nb = (n_words + 1) / 2;
    std::vector<uint64_t> w(n_words + 1, 0xA5A5A5A5A5A5A5A5ull);   // a guard word after the request
    aes_ctr_keystream(job, w.data(), n_words);
    CHECK(w[n_words] == 0xA5A5A5A5A5A5A5A5ull, "keystream of %zu words wrote past its end", n_words);
    return hex(w.data(), 8 * n_words);
}

static void check_vectors() {
    // FIPS-197 C.3: the plaintext as the counter block
    CHECK(keystream_hex("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f", "00112233445566778899aabbccddeeff", 2) ==
              "8ea2b7ca516745bfeafc49904b496089",
          "FIPS-197 C.3");
    // SP 800-38A F.5.5 as one stream from f0f1..feff (crosses a byte carry)
    const char* key = "603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4";
    const std::string ks = keystream_hex(key, "f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff", 8);
    CHECK(ks == "0bdf7df1591716335e9a8b15c860c5025a6e699d536119065433863c8f657b94"
                "1bc12c9c01610d5d0d8bd6a3378eca622956e1c8693536b1bee99c73a31576b6",
          "SP 800-38A F.5.5: %s", ks.c_str());
    CHECK(keystream_hex(key, "f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff", 7) == ks.substr(0, 112), "an odd request is a prefix");
    // V = 2^128 - 2: blocks fe, ff, 00, 01 (the same blocks asked for one by one)
    const std::string wrap = keystream_hex(key, "fffffffffffffffffffffffffffffffe", 8);
    CHECK(wrap.substr(32, 32) == keystream_hex(key, "ffffffffffffffffffffffffffffffff", 2), "wrap: block 2^128 - 1");
    CHECK(wrap.substr(64, 32) == keystream_hex(key, "00000000000000000000000000000000", 2), "wrap: block 0");
    CHECK(wrap.substr(96, 32) == keystream_hex(key, "00000000000000000000000000000001", 2), "wrap: block 1");
    // the carry into the high half
    const std::string half = keystream_hex(key, "0000000000000005ffffffffffffffff", 4);
    CHECK(half.substr(32, 32) == keystream_hex(key, "00000000000000060000000000000000", 2), "carry into the high half");
}

struct fake_source {
    int calls = 0;
    int fail_at = -1;   // the call (from 1) that fails
    int operator()(uint8_t out[kDrbgSeedLen]) {
        ++calls;
        if (calls == fail_at) return -1;
        for (size_t i = 0; i < kDrbgSeedLen; ++i) out[i] = (uint8_t)(calls * 16 + i);
        return 0;
    }
};

static void check_seeding() {
    uint64_t w[8], cnt[4];
    {   // self-seeding: lazily at first use, then a reseed exactly when `interval` calls have run
        fake_source src;
        ctr_drbg g(3, [&](uint8_t* e) { return src(e); });
        g.counts(cnt);
        CHECK(src.calls == 0 && cnt[3] == 0, "nothing is drawn before the first use");
        CHECK(g.generate(w, 0) == 0 && src.calls == 0, "a zero request does not seed");
        CHECK(g.generate(w, 3) == 0 && src.calls == 1, "first use seeds: %d", src.calls);
        CHECK(g.generate(w, 1) == 0 && g.generate(w, 2) == 0 && src.calls == 1, "calls 2, 3 draw nothing: %d", src.calls);
        CHECK(g.generate(w, 0) == 0 && src.calls == 1, "a zero request is not counted");
        g.counts(cnt);
        CHECK(cnt[0] == 3 && cnt[1] == 4 && cnt[2] == 0 && cnt[3] == 1, "counts %llu %llu %llu %llu", (unsigned long long)cnt[0],
              (unsigned long long)cnt[1], (unsigned long long)cnt[2], (unsigned long long)cnt[3]);
        CHECK(g.generate(w, 2) == 0 && src.calls == 2, "call 4 reseeds first: %d", src.calls);
        CHECK(g.generate(w, 2) == 0 && g.generate(w, 2) == 0 && src.calls == 2, "calls 5, 6: %d", src.calls);
        CHECK(g.generate(w, 2) == 0 && src.calls == 3, "call 7 reseeds: %d", src.calls);
        g.counts(cnt);
        CHECK(cnt[0] == 7 && cnt[2] == 2, "7 calls, 2 reseeds: %llu %llu", (unsigned long long)cnt[0], (unsigned long long)cnt[2]);
        // the self-seeded stream is the explicit one of the same entropy
        fake_source again;
        uint8_t e1[kDrbgSeedLen], e2[kDrbgSeedLen];
        again(e1);
        again(e2);
        ctr_drbg x(3, [](uint8_t*) { return -1; });
        uint64_t v[8];
        CHECK(x.seed(e1) == 0, "explicit seed");
        x.generate(v, 3);
        x.generate(v, 1);
        x.generate(v, 2);
        CHECK(x.reseed(e2) == 0, "explicit reseed");
        x.generate(v, 2);
        fake_source s3;
        ctr_drbg y(3, [&](uint8_t* e) { return s3(e); });
        y.generate(w, 3);
        y.generate(w, 1);
        y.generate(w, 2);
        y.generate(w, 2);
        CHECK(w[0] == v[0] && w[1] == v[1], "a reseed at the interval is update(entropy)");
    }
    {   // an explicitly seeded instance never calls the source
        fake_source src;
        ctr_drbg g(2, [&](uint8_t* e) { return src(e); });
        uint8_t seed[kDrbgSeedLen] = {1, 2, 3};
        CHECK(g.seed(seed) == 0, "seed");
        for (int i = 0; i < 9; ++i) g.generate(w, 5);
        uint8_t b[48];
        g.generate_host(b, sizeof b);
        g.counts(cnt);
        CHECK(src.calls == 0 && cnt[0] == 10 && cnt[2] == 0 && cnt[3] == 0, "explicit seed: %d source calls", src.calls);
    }
    {   // the source failing: at the first use, and at a reseed; the state is not advanced
        fake_source src;
        src.fail_at = 1;
        ctr_drbg g(1, [&](uint8_t* e) { return src(e); });
        CHECK(g.generate(w, 2) == PVAC_EDEVICE, "no entropy at first use");
        CHECK(g.seed(nullptr) == 0, "the source works again");
        CHECK(g.generate(w, 2) == 0, "call 1");
        src.fail_at = src.calls + 1;
        g.counts(cnt);
        CHECK(g.generate(w, 2) == PVAC_EDEVICE, "no entropy at the reseed");
        uint64_t after[4];
        g.counts(after);
        CHECK(after[0] == cnt[0] && after[1] == cnt[1] && after[2] == cnt[2], "a failed request counts nothing");
        CHECK(g.reseed(nullptr) == 0 && g.generate(w, 2) == 0, "recovers once the source does");
        ctr_drbg none(1, nullptr);
        CHECK(none.generate(w, 1) == PVAC_EDEVICE, "no source at all");
    }
    {   // generate_host and device-split requests advance one shared block counter
        ctr_drbg g;
        uint8_t seed[kDrbgSeedLen] = {9};
        g.seed(seed);
        uint64_t first = 99;
        aes_ctr_job job;
        uint8_t b[20];
        CHECK(g.request(5, &job, &first) == 0 && first == 0 && job.nb == 3, "device request 1");
        CHECK(g.generate_host(b, 20, &first) == 0 && first == 3, "host request follows: %llu", (unsigned long long)first);
        CHECK(g.request(0, &job, &first) == 0 && job.nb == 0 && first == 5, "a zero request hands out nothing");
        CHECK(g.request(2, &job, &first) == 0 && first == 5 && job.nb == 1, "device request 2: %llu", (unsigned long long)first);
        g.counts(cnt);
        CHECK(cnt[0] == 3 && cnt[1] == 6, "3 calls, 6 blocks");
        wipe(&job, sizeof job);
    }
    {   // the real source
        ctr_drbg a, b;
        uint64_t x[4], y[4];
        CHECK(a.generate(x, 4) == 0 && b.generate(y, 4) == 0, "getrandom");
        CHECK(x[0] != y[0] || x[1] != y[1], "two self-seeded instances differ");
        a.counts(cnt);
        CHECK(cnt[3] == 1, "self-seeded");
    }
}

static int run_script(const char* path) {
    std::ifstream in(path);
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", path);
        return 2;
    }
    ctr_drbg g(kDrbgReseedInterval, [](uint8_t*) { return -1; });   // the script seeds it: the source is never needed
    std::string line;
    int ln = 0, ops = 0;
    while (std::getline(in, line)) {
        ++ln;
        std::istringstream ss(line);
        std::string op, a, b;
        ss >> op >> a >> b;
        if (op.empty()) continue;
        if (b == "-") b.clear();   // an empty output
        ++ops;
        if (op == "seed") {
            CHECK(g.seed(unhex(a).data()) == 0, "line %d: seed", ln);
        } else if (op == "reseed") {
            CHECK(g.reseed(unhex(a).data()) == 0, "line %d: reseed", ln);
        } else if (op == "gen" || op == "dev") {
            const size_t n = std::strtoull(a.c_str(), nullptr, 10);
            std::vector<uint64_t> w(n + 1, 0x5A5A5A5A5A5A5A5Aull);
            if (op == "gen") {
                CHECK(g.generate(w.data(), n) == 0, "line %d: generate", ln);
            } else {
                aes_ctr_job job;
                CHECK(g.request(n, &job) == 0 && job.nb == (n + 1) / 2, "line %d: request", ln);
                aes_ctr_keystream(job, w.data(), n);
                wipe(&job, sizeof job);
            }
            CHECK(w[n] == 0x5A5A5A5A5A5A5A5Aull, "line %d: wrote past %zu words", ln, n);
            CHECK(hex(w.data(), 8 * n) == b, "line %d: %s of %zu words differs from the model", ln, op.c_str(), n);
        } else if (op == "host") {
            const size_t k = std::strtoull(a.c_str(), nullptr, 10);
            std::vector<uint8_t> o(k + 1, 0x5A);
            CHECK(g.generate_host(o.data(), k) == 0, "line %d: generate_host", ln);
            CHECK(o[k] == 0x5A && hex(o.data(), k) == b, "line %d: generate_host of %zu bytes differs from the model", ln, k);
        } else if (op == "counts") {
            std::string c, d;
            ss >> c >> d;
            uint64_t cnt[4];
            g.counts(cnt);
            CHECK(cnt[0] == std::strtoull(a.c_str(), nullptr, 10) && cnt[1] == std::strtoull(b.c_str(), nullptr, 10) &&
                      cnt[2] == std::strtoull(c.c_str(), nullptr, 10) && cnt[3] == std::strtoull(d.c_str(), nullptr, 10),
                  "line %d: counts %llu %llu %llu %llu", ln, (unsigned long long)cnt[0], (unsigned long long)cnt[1],
                  (unsigned long long)cnt[2], (unsigned long long)cnt[3]);
        } else {
            CHECK(false, "line %d: unknown operation %s", ln, op.c_str());
        }
    }
    CHECK(ops > 0, "an empty script");
    return 0;
}

static void check_threads() {
    constexpr int kThreads = 4, kCalls = 400;
    ctr_drbg g;
    uint8_t seed[kDrbgSeedLen] = {7};
    g.seed(seed);
    std::vector<std::vector<std::pair<uint64_t, uint64_t>>> got(kThreads);   // (first block, blocks)
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; ++t)
        th.emplace_back([&, t] {
            for (int i = 0; i < kCalls; ++i) {
                uint8_t b[64];
                const size_t bytes = 1 + (size_t)((t * 31 + i * 7) % 64);
                uint64_t first = 0;
                if (g.generate_host(b, bytes, &first) != 0) return;
                got[t].emplace_back(first, ((bytes + 7) / 8 + 1) / 2);
            }
        });
    for (std::thread& t : th) t.join();
    std::vector<uint8_t> seen;
    uint64_t total = 0;
    for (auto& v : got) {
        CHECK(v.size() == (size_t)kCalls, "a thread stopped early");
        for (auto& r : v) total += r.second;
    }
    seen.assign(total, 0);
    for (auto& v : got)
        for (auto& r : v)
            for (uint64_t k = 0; k < r.second; ++k) {
                CHECK(r.first + k < total && !seen[r.first + k], "block index %llu handed out twice", (unsigned long long)(r.first + k));
                if (r.first + k < total) seen[r.first + k] = 1;
            }
    uint64_t cnt[4];
    g.counts(cnt);
    CHECK(cnt[0] == (uint64_t)kThreads * kCalls && cnt[1] == total, "counts after the threads");
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: drbg_check <script> | threads\n");
        return 2;
    }
    if (std::string(argv[1]) == "threads") {
        check_threads();
    } else {
        check_vectors();
        check_seeding();
        const int rc = run_script(argv[1]);
        if (rc) return rc;
    }
    if (g_fail) {
        std::printf("drbg_check: %d failed\n", g_fail);
        return 1;
    }
    std::printf("drbg_check: ok\n");
    return 0;
}
