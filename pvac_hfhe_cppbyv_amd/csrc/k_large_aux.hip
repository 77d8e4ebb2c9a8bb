// k_large_aux.hip — kernels of the general ct_mul path (k_mul_large.hip) that run outside its launch
// sequence: the static bucket groups the host builds once per (bucket count, B), and the dense chain
// images turned back into hash-order records.
#include "k_large.hpp"

#include <algorithm>

namespace pvhip {

namespace {

// ---------------------------------------------------------------- static bucket groups
__global__ __launch_bounds__(kLB) void k_grp_insert(fastmod64 nbm, uint32_t Bm, uint64_t S, uint32_t hbits,
                                                    uint32_t* head, uint32_t* next, unsigned long long* tkeyb,
                                                    uint32_t* thead) {
    const uint64_t hmask = (1ull << hbits) - 1;
    for (uint64_t s = (uint64_t)blockIdx.x * kLB + threadIdx.x; s < S; s += (uint64_t)gridDim.x * kLB) {
        const uint64_t lp = s / Bm, r = s - lp * Bm;
        const uint64_t b = fmod64(((lp << 32) | r) * kGolden, nbm);   // std::hash -> bucket
        uint64_t h = ((b + 1) * kGolden) >> (64 - hbits);
        for (;;) {
            const unsigned long long prev = atomicCAS(&tkeyb[h], 0ull, (unsigned long long)(b + 1));
            if (prev == 0ull || prev == b + 1) break;
            h = (h + 1) & hmask;
        }
        next[s] = atomicExch(&thead[h], (uint32_t)(s + 1));
        head[s] = (uint32_t)h;
    }
}

__global__ __launch_bounds__(kLB) void k_grp_finish(uint64_t S, uint32_t* head, const uint32_t* next,
                                                    const uint32_t* thead) {
    for (uint64_t s = (uint64_t)blockIdx.x * kLB + threadIdx.x; s < S; s += (uint64_t)gridDim.x * kLB) {
        const uint32_t h0 = thead[head[s]];
        head[s] = (h0 == (uint32_t)(s + 1) && next[s] == 0u) ? 0u : h0;   // 0: alone in its bucket
    }
}

}  // namespace

hipError_t launch_grp_build(fastmod64 nbm, uint32_t Bm, uint64_t S, uint32_t hbits, uint32_t* head, uint32_t* next,
                            unsigned long long* tmp_key, uint32_t* tmp_head, hipStream_t st) {
    if (!S) return hipSuccess;
    const unsigned gs = grid_x(S, kLB * 2, 4096);
    hipLaunchKernelGGL(k_grp_insert, dim3(gs), dim3(kLB), 0, st, nbm, Bm, S, hbits, head, next, tmp_key, tmp_head);
    hipLaunchKernelGGL(k_grp_finish, dim3(gs), dim3(kLB), 0, st, S, head, (const uint32_t*)next,
                       (const uint32_t*)tmp_head);
    return hipGetLastError();
}

// ---------------------------------------------------------------- dense chain images -> records
// (k_large_products_direct's image writer; see mul_large_args::A_img) Listed pair y (pairs[y], its
// edges at tmp + 3 pairs[n + y]): the image is copied out, then every slot's edge is written back at
// its hash-order position as (meta, w_lo, w_hi); the flags are cleared last. A launch covers the
// listed pairs y = y0 + blockIdx.y (grid y is capped, so a long list takes several launches).
__global__ __launch_bounds__(256) void k_img_copy(pvac_ct_batch A, const uint32_t* img, const uint64_t* pairs, uint32_t n,
                                                  uint32_t y0, uint64_t* tmp) {
    const uint32_t y = y0 + blockIdx.y;
    const uint64_t pr = pairs[y];
    if (!img[pr]) return;
    const uint64_t eo = A.e_off[pr], ne = A.e_cnt[pr];
    uint64_t* t = tmp + 3u * pairs[n + y];
    const uint32_t* ids = (const uint32_t*)(A.meta + eo);
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < ne; k += (uint64_t)gridDim.x * 256u) {
        t[3u * k] = ids[k];
        t[3u * k + 1u] = A.w_lo[eo + k];
        t[3u * k + 2u] = A.w_hi[eo + k];
    }
}
__global__ __launch_bounds__(256) void k_img_scatter(pvac_ct_batch A, const uint32_t* img, const uint64_t* pairs, uint32_t n,
                                                     uint32_t y0, const uint64_t* tmp, uint32_t Bm) {
    const uint32_t y = y0 + blockIdx.y;
    const uint64_t pr = pairs[y];
    if (!img[pr]) return;
    const uint64_t eo = A.e_off[pr], ne = A.e_cnt[pr];
    const uint64_t slab = 2u * Bm, first = A.l_cnt[pr] - ne / slab;   // the slabs are the last layers
    const uint64_t* t = tmp + 3u * pairs[n + y];
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < ne; k += (uint64_t)gridDim.x * 256u) {
        const uint32_t id = (uint32_t)t[3u * k];
        const uint32_t pos = id & 0x1FFFFFu, cell = id >> 21;
        if (pos >= ne) continue;   // not an image slot (never written by the image writer)
        const uint32_t ch = cell >= Bm ? 1u : 0u;
        A.meta[eo + pos] = make_meta((uint32_t)(first + k / slab), cell - ch * Bm, ch);
        A.w_lo[eo + pos] = t[3u * k + 1u];
        A.w_hi[eo + pos] = t[3u * k + 2u];
    }
}
__global__ __launch_bounds__(64) void k_img_clear(uint32_t* img, const uint64_t* pairs, uint32_t n) {
    const uint32_t y = blockIdx.x * 64u + threadIdx.x;
    if (y < n) img[pairs[y]] = 0u;
}
hipError_t launch_image_to_records(const pvac_ct_batch& A, uint32_t* img, const uint64_t* pairs, uint32_t n_pairs,
                                   uint64_t* tmp, uint32_t Bm, uint32_t y_cap, hipStream_t st) {
    if (!n_pairs) return hipSuccess;
    y_cap = std::min<uint32_t>(std::max<uint32_t>(y_cap, 1u), 65535u);   // grid y limit (tests pass small caps)
    for (uint32_t y0 = 0; y0 < n_pairs; y0 += y_cap) {
        const uint32_t ny = std::min<uint32_t>(n_pairs - y0, y_cap);
        hipLaunchKernelGGL(k_img_copy, dim3(64, ny), dim3(256), 0, st, A, img, pairs, n_pairs, y0, tmp);
        hipLaunchKernelGGL(k_img_scatter, dim3(64, ny), dim3(256), 0, st, A, img, pairs, n_pairs, y0, tmp, Bm);
    }
    hipLaunchKernelGGL(k_img_clear, dim3((n_pairs + 63u) / 64u), dim3(64), 0, st, img, pairs, n_pairs);
    return hipGetLastError();
}

}  // namespace pvhip
