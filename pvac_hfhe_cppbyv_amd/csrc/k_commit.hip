// k_commit.hip — batched commit_ct (ops/commit.hpp:12-88): one SHA-256 per cipher over the message
// commit_msg.hpp states. SHA-256 is a serial chain within a cipher, so the parallelism is across
// ciphers: one cipher per lane, each lane's feeder staging its words in a 32-word LDS ring, and one
// compression per loop trip for every lane that has a block (the lanes differ only in where their
// messages stand, never in which branch calls the compression).
//
// Ragged batches: a lane that has written its digest takes the next cipher index from a counter, so a
// wave costs the sum of what its lanes drew, not 64 x its longest cipher; digests go out by cipher
// index. Small batches: a wave's instruction time does not depend on how many of its lanes are active,
// and waves that share a CU slow each other down, most of all when few of their lanes are active
// (64 products with sigma as 16 workgroups of four one-lane waves: 222 ms; as 64 one-wave workgroups on
// 64 CUs: 88 ms, the time of one chain). So launch_commit_ct gives every CU one wave,
// fills its 64 lanes, and only then adds waves to a CU, up to 16. Where the waves land is not left to
// the dispatcher: a workgroup holds all the waves of its CU and asks for more than half a CU's LDS, so
// exactly one workgroup runs on a CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "commit_msg.hpp"
#include "common.hpp"

namespace pvhip {

namespace {

constexpr int kCommitMaxWaves = 16;             // per workgroup: 4 per SIMD (101 VGPRs allow no more)
constexpr size_t kCommitRingBytes = kCommitRingWords * 64 * sizeof(uint32_t);   // one wave's rings: 8 KiB
constexpr size_t kCommitLdsFloor = 96 * 1024;   // of a CU's 160 KiB: a second workgroup does not fit

// ring word i of lane l lives at word i * 64 + l: whatever word index a lane is at, its bank is its lane
struct commit_lds_ring {
    uint32_t* base;
    __device__ __forceinline__ void put(uint32_t i, uint32_t w) { base[i * 64] = w; }
    __device__ __forceinline__ uint32_t get(uint32_t i) const { return base[i * 64]; }
};

struct commit_args {
    pvac_ct_batch X;
    uint32_t head[kCommitHeadWords];
    uint32_t sigma_bytes;
    uint32_t lanes;
    unsigned long long* counter;
    uint8_t* out;
};

__global__ __launch_bounds__(64 * kCommitMaxWaves) void k_commit_ct(const commit_args a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ring_words[];   // [waves][kCommitRingWords][64]
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;   // the waves never meet: no barrier below
    commit_lds_ring ring{ring_words + wave * kCommitRingWords * 64 + lane};
    commit_feeder<commit_lds_ring> f;
    f.reset();
    commit_cipher c{};
    sha_state st;
    sha_init(st);
    uint64_t cur = 0;
    bool more = lane < a.lanes;
    for (;;) {
        if (more && f.idle()) {
            cur = atomicAdd(a.counter, 1ull);
            if (cur < a.X.n) {
                c = commit_cipher_of(a.X, cur, a.sigma_bytes);
                sha_init(st);
                f.begin(ring, a.head, c);
            } else {
                more = false;
            }
        }
        f.fill_block(ring, c);
        const bool have = f.ready();
        if (!__any(have)) break;
        if (have) {
            uint32_t blk[16];
            f.take(ring, blk);
            sha_compress(st, blk);
            if (f.idle()) {
                uint8_t* o = a.out + 32 * cur;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    o[4 * i] = (uint8_t)(st.h[i] >> 24);
                    o[4 * i + 1] = (uint8_t)(st.h[i] >> 16);
                    o[4 * i + 2] = (uint8_t)(st.h[i] >> 8);
                    o[4 * i + 3] = (uint8_t)st.h[i];
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_commit_ct(const pvac_ct_batch& X, const uint32_t head[kCommitHeadWords], uint32_t sigma_bytes,
                            int num_cus, unsigned long long* counter, uint8_t* out, hipStream_t st) {
    if (!X.n) return hipSuccess;
    hipError_t e = hipMemsetAsync(counter, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    commit_args a{};
    a.X = X;
    for (uint32_t i = 0; i < kCommitHeadWords; ++i) a.head[i] = head[i];
    a.sigma_bytes = sigma_bytes;
    const uint64_t cus = (uint64_t)std::max(num_cus, 1);
    // waves per CU: one until its 64 lanes are full, then as many as the batch fills, 16 at most (past
    // that the counter deals the rest to the lanes that finish); the lanes of a wave share what is left
    const uint64_t group = std::min<uint64_t>((X.n + 64 * cus - 1) / (64 * cus), kCommitMaxWaves);
    a.lanes = (uint32_t)std::min<uint64_t>(64, (X.n + group * cus - 1) / (group * cus));
    a.counter = counter;
    a.out = out;
    const uint64_t per_group = group * a.lanes;
    const uint64_t grid = std::min<uint64_t>((X.n + per_group - 1) / per_group, cus);
    const size_t lds = std::max<size_t>(group * kCommitRingBytes, kCommitLdsFloor);
    hipLaunchKernelGGL(k_commit_ct, dim3((unsigned)grid), dim3((unsigned)(64 * group)), lds, st, a);
    return hipGetLastError();
}

}  // namespace pvhip
