// k_ct_image.hip — the device .ct codec: a resident batch <-> a byte-exact .ct file image in device
// memory (geometry, stream words and validation: ct_image.hpp; the host codec ct_codec.cpp is the
// specification).
//
// Work unit of the edge kernels: a tile = up to ept whole edge records of one cipher (at most 16 KiB of
// image). Tiles are numbered through the batch (toff = exclusive scan of the per-cipher tile counts) and
// dealt to workgroups from that list, so one 345 K-edge cipher and 2^20 small ones both fill the device.
//
// Write: a workgroup stages its tile's stream words in LDS with wide loads (8 bytes for meta / w_lo /
// w_hi, 16 or 8 bytes for sigma rows), then every lane assembles aligned 16-byte granules from five
// consecutive staged words with a byte funnel shift and stores them whole. A tile starts and ends
// mid-granule (its neighbours belong to other workgroups): the ragged first and last granule are
// written with 1-, 2-, 4- and 8-byte stores of exactly the tile's own bytes. No byte is written twice
// and no store is misaligned. Layer records (under 4 % of an image) go out byte by byte, one wave per
// cipher with a scan over the record sizes.
//
// Parse: the inverse, output-driven over the SoA words and the 16- or 8-byte pieces of the sigma rows;
// each piece comes from aligned image dwords, funnel-shifted, and goes out in one aligned store. The
// row kernels read the validation pass's verdict from device memory (the ctl words) and write nothing
// unless every cipher is well-formed and the totals fit, so the call synchronises once, at its end.
#include <algorithm>

#include "common.hpp"
#include "ct_image.hpp"

namespace pvhip {

namespace {

constexpr int kImgBlock = 256;
// LDS words of the edge writer for tiles of at most ne edges: the tile's words, the lead (<= 4) and the
// zeros a last granule reads (4 ng <= words + 7)
inline uint32_t ct_image_lds_words(uint32_t ne, const ct_geom& g) { return ne * g.wpe + 8; }

// largest i < n with toff[i] <= t: the cipher tile t belongs to (ciphers without tiles share an offset
// with their successor and are never found)
__device__ __forceinline__ uint64_t tile_cipher(const uint64_t* __restrict__ toff, uint64_t n, uint64_t t) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (toff[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t pick4(const uint32_t v[4], uint32_t k) {
    return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3];
}

// bytes [lo, hi) of the granule at p (16-byte aligned) from its four words: naturally aligned stores
// of 8, 4, 2 and 1 bytes, each byte once
__device__ __forceinline__ void store_granule_part(uint8_t* p, const uint32_t v[4], uint32_t lo, uint32_t hi) {
    uint32_t o = lo;
    while (o < hi) {
        uint32_t s = 8;
        while ((o & (s - 1)) || o + s > hi) s >>= 1;
        const uint32_t w = pick4(v, o >> 2);
        if (s == 8) *(uint64_t*)(p + o) = (uint64_t)w | (uint64_t)pick4(v, (o >> 2) + 1) << 32;
        else if (s == 4) *(uint32_t*)(p + o) = w;
        else if (s == 2) *(uint16_t*)(p + o) = (uint16_t)(w >> (8 * (o & 3)));
        else p[o] = (uint8_t)(w >> (8 * (o & 3)));
        o += s;
    }
}

// ---------------------------------------------------------------- write: plan
// sz[i] = bytes of cipher i in the image; 8 lanes per cipher share its layers
__global__ __launch_bounds__(kImgBlock) void k_img_sizes(pvac_ct_batch X, ct_geom g, uint64_t* __restrict__ sz,
                                                          unsigned long long* __restrict__ ctl) {
    const uint64_t i = ((uint64_t)blockIdx.x * kImgBlock + threadIdx.x) >> 3;
    const uint32_t sub = threadIdx.x & 7u;
    uint64_t b = 0;
    uint32_t bad = 0;
    if (i < X.n) b = ct_layer_bytes_sum(X.layers + X.l_off[i], sub, X.l_cnt[i], 8, &bad);
    for (int d = 1; d < 8; d <<= 1) b += __shfl_xor(b, d, 64);
    if (bad) atomicAdd(&ctl[2], (unsigned long long)bad);
    if (i < X.n && sub == 0) sz[i] = kCtCipherHdr + b + X.e_cnt[i] * g.eb();
}

// pos from the scanned sizes (ctl[0] = their total), the per-cipher tile counts and, in ctl[3], the
// edges of the batch's largest tile (the edge writer's LDS is sized by it)
__global__ __launch_bounds__(kImgBlock) void k_img_pos(pvac_ct_batch X, ct_geom g, const uint64_t* __restrict__ sz,
                                                        unsigned long long* __restrict__ ctl, uint64_t* __restrict__ pos,
                                                        uint64_t* __restrict__ tcnt) {
    const uint64_t i = (uint64_t)blockIdx.x * kImgBlock + threadIdx.x;
    uint32_t ne = 0;   // edges of cipher i's largest tile
    if (i < X.n) {
        const uint64_t E = X.e_cnt[i];
        pos[i] = kCtFileHdr + sz[i];
        tcnt[i] = (E + g.ept - 1) / g.ept;
        ne = (uint32_t)(E < g.ept ? E : g.ept);
    } else if (i == X.n) {
        pos[i] = kCtFileHdr + ctl[0];
    }
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_xor(ne, d, 64);
        ne = o > ne ? o : ne;
    }
    if ((threadIdx.x & 63) == 0 && ne) atomicMax(&ctl[3], (unsigned long long)ne);
}

// ---------------------------------------------------------------- write: headers and layers
// block i < n: cipher i's count words and layer records; block n: the file header
__global__ __launch_bounds__(64) void k_img_heads(pvac_ct_batch X, const uint64_t* __restrict__ pos, uint8_t* __restrict__ image) {
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    if (i == X.n) {
        if (lane == 0) *(uint4*)image = make_uint4(kCtMagic, kCtVersion, (uint32_t)X.n, (uint32_t)(X.n >> 32));
        return;
    }
    const uint64_t nL = (uint32_t)X.l_cnt[i], nE = (uint32_t)X.e_cnt[i];
    uint64_t off = pos[i];
    if (lane < 8) image[off + lane] = (uint8_t)((lane < 4 ? nL : nE) >> (8 * (lane & 3)));
    off += kCtCipherHdr;
    const pvac_layer* L = X.layers + X.l_off[i];
    for (uint64_t c = 0; c < nL; c += 64) {
        pvac_layer y{};
        uint32_t size = 0;
        if (c + lane < nL) {
            y = L[c + lane];
            size = ct_layer_bytes(y.rule);
        }
        const uint32_t incl = wave_incl_scan_u32(size);
        uint8_t* o = image + off + (incl - size);
        for (uint32_t k = 0; k < size; ++k) o[k] = ct_layer_byte(y, k);
        off += __builtin_amdgcn_readlane(incl, 63);
    }
}

// ---------------------------------------------------------------- write: edges (the hot kernel)
template <bool WIDE>
__global__ __launch_bounds__(kImgBlock) void k_img_edges_write(pvac_ct_batch X, ct_geom g, const uint64_t* __restrict__ pos,
                                                                const uint64_t* __restrict__ toff, uint64_t ntiles,
                                                                uint32_t max_ne, uint8_t* __restrict__ image) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sw[];   // ct_image_lds_words(largest tile) words
    const uint32_t tid = threadIdx.x;
    const uint32_t pp = 3u + (WIDE ? g.nw / 2u : g.nw);   // staged pieces per edge
    const uint64_t eb = g.eb();
    // a workgroup takes a run of consecutive tiles: one search, then the cipher index only moves forward
    const uint64_t per = (ntiles + gridDim.x - 1) / gridDim.x;
    uint64_t t = blockIdx.x * per;
    const uint64_t t1 = t + per < ntiles ? t + per : ntiles;
    if (t >= t1) return;
    uint64_t i = tile_cipher(toff, X.n, t);
    for (; t < t1; ++t) {
        while (i + 1 < X.n && toff[i + 1] <= t) ++i;
        const uint64_t E = X.e_cnt[i];
        const uint64_t ea = (t - toff[i]) * g.ept;                    // the tile's first edge
        const uint32_t ne = (uint32_t)(E - ea < g.ept ? E - ea : g.ept);   // ... and its edge count
        if (ne > max_ne) continue;   // not the batch that was planned: its LDS was sized for max_ne edges
        const uint64_t bs = pos[i + 1] - (E - ea) * eb, be = bs + (uint64_t)ne * eb;   // its bytes in the image
        const uint64_t a0 = bs & ~15ull;                              // its first granule
        const int32_t s0 = (int32_t)(a0 - bs);                        // -15 .. 0
        const uint32_t lead = (uint32_t)(-(s0 >> 2));                 // staged word j sits at sw[lead + j]
        const uint32_t r = (uint32_t)s0 & 3u;
        const uint32_t nwords = ne * g.wpe;
        const uint32_t ng = (uint32_t)((be - a0 + 15) >> 4);
        // zeros around the staged words: a granule reads sw[4 gi .. 4 gi + 4]
        if (tid < lead) sw[tid] = 0;
        for (uint32_t k = lead + nwords + tid; k < 4 * ng + 1; k += kImgBlock) sw[k] = 0;
        const uint64_t slot = X.e_off[i] + ea;
        const uint64_t* __restrict__ meta = X.meta + slot;
        const uint64_t* __restrict__ wlo = X.w_lo + slot;
        const uint64_t* __restrict__ whi = X.w_hi + slot;
        const uint64_t* __restrict__ sig = g.nw ? X.sigma + slot * X.sigma_words : nullptr;
        for (uint32_t x = tid; x < ne * pp; x += kImgBlock) {
            const uint32_t e = x / pp, p = x - e * pp;
            uint32_t* d = sw + lead + e * g.wpe;
            if (p == 0) {
                const uint64_t m = meta[e];
                d[0] = (uint32_t)m;
                d[1] = (uint32_t)(m >> 32) & 0xFFFFFFu;
            } else if (p == 1) {
                const uint64_t w = wlo[e];
                d[2] = (uint32_t)w;
                d[3] = (uint32_t)(w >> 32);
            } else if (p == 2) {
                const uint64_t w = whi[e];
                d[4] = (uint32_t)w;
                d[5] = (uint32_t)(w >> 32);
                d[6] = g.nbits;
            } else if (WIDE) {
                const uint32_t q = p - 3;
                const uint4 v = *(const uint4*)(sig + (uint64_t)e * X.sigma_words + 2 * q);
                d[7 + 4 * q] = v.x;
                d[8 + 4 * q] = v.y;
                d[9 + 4 * q] = v.z;
                d[10 + 4 * q] = v.w;
            } else {
                const uint32_t q = p - 3;
                const uint64_t w = sig[(uint64_t)e * X.sigma_words + q];
                d[7 + 2 * q] = (uint32_t)w;
                d[8 + 2 * q] = (uint32_t)(w >> 32);
            }
        }
        __syncthreads();
        for (uint32_t gi = tid; gi < ng; gi += kImgBlock) {
            const uint4 q = *(const uint4*)(sw + 4 * gi);
            const uint32_t w4 = sw[4 * gi + 4];
            uint32_t v[4];
            v[0] = ct_funnel(q.x, q.y, r);
            v[1] = ct_funnel(q.y, q.z, r);
            v[2] = ct_funnel(q.z, q.w, r);
            v[3] = ct_funnel(q.w, w4, r);
            const uint64_t a = a0 + 16ull * gi;
            uint8_t* p = image + a;
            if (a >= bs && a + 16 <= be) {
                *(uint4*)p = make_uint4(v[0], v[1], v[2], v[3]);
            } else {
                const uint32_t lo = a < bs ? (uint32_t)(bs - a) : 0u;
                const uint32_t hi = a + 16 > be ? (uint32_t)(be - a) : 16u;
                store_granule_part(p, v, lo, hi);
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- parse: plan
// ctl words of a parse: 0 / 1 layer and edge totals, 2 tiles, 3 malformed ciphers, 4 edges whose
// nbits differs
__device__ __forceinline__ bool parse_go(const unsigned long long* ctl, uint64_t layer_cap, uint64_t edge_cap) {
    return ctl[3] == 0 && ctl[0] <= layer_cap && ctl[1] <= edge_cap;
}

// one lane per cipher: validation, counts (twice: one copy is scanned into offsets), tile counts
__global__ __launch_bounds__(kImgBlock) void k_img_validate(const uint32_t* __restrict__ img32, uint64_t len,
                                                             const uint64_t* __restrict__ pos, uint64_t n, ct_geom g,
                                                             uint32_t* __restrict__ status, uint64_t* __restrict__ cL,
                                                             uint64_t* __restrict__ cE, uint64_t* __restrict__ oL,
                                                             uint64_t* __restrict__ oE, uint64_t* __restrict__ tcnt,
                                                             unsigned long long* __restrict__ ctl) {
    const uint64_t i = (uint64_t)blockIdx.x * kImgBlock + threadIdx.x;
    if (n == 0) {   // no cipher to blame: the image must be the bare header
        if (i == 0 && (pos[0] != kCtFileHdr || len != kCtFileHdr)) atomicAdd(&ctl[3], 1ull);
        return;
    }
    if (i >= n) return;
    uint64_t nL, nE;
    const uint32_t st = ct_parse_validate(img32, len, pos, n, i, g, &nL, &nE);
    if (status) status[i] = st;
    if (st) atomicAdd(&ctl[3], 1ull);
    cL[i] = oL[i] = nL;
    cE[i] = oE[i] = nE;
    tcnt[i] = (nE + g.ept - 1) / g.ept;
}

// ---------------------------------------------------------------- parse: index arrays and layers
__device__ __forceinline__ uint64_t image_u64_bytes(const uint8_t* __restrict__ p) {
    uint64_t x = 0;
    for (int k = 0; k < 8; ++k) x |= (uint64_t)p[k] << (8 * k);
    return x;
}

// one wave per cipher: its four index words, then 64 layers at a time: every lane walks the 64 rule
// bytes (record starts are serial by construction), lane k keeps record k's start and decodes it
__global__ __launch_bounds__(64) void k_img_layers_parse(const uint8_t* __restrict__ image, const uint64_t* __restrict__ pos,
                                                          const uint64_t* __restrict__ cL, const uint64_t* __restrict__ cE,
                                                          const uint64_t* __restrict__ oL, const uint64_t* __restrict__ oE,
                                                          pvac_ct_batch X, const unsigned long long* __restrict__ ctl,
                                                          uint64_t layer_cap, uint64_t edge_cap) {
    if (!parse_go(ctl, layer_cap, edge_cap)) return;
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint64_t nL = cL[i], lo = oL[i];
    if (lane == 0) {
        X.l_off[i] = lo;
        X.l_cnt[i] = nL;
        X.e_off[i] = oE[i];
        X.e_cnt[i] = cE[i];
    }
    uint64_t off = pos[i] + kCtCipherHdr;
    for (uint64_t c = 0; c < nL; c += 64) {
        const uint32_t m = (uint32_t)(nL - c < 64 ? nL - c : 64);
        uint64_t my = 0;
        uint32_t rule = 0;
        for (uint32_t k = 0; k < m; ++k) {
            const uint32_t rb = image[off];
            if (lane == k) {
                my = off;
                rule = rb;
            }
            off += ct_layer_bytes(rb);
        }
        if (lane < m) {
            pvac_layer y{};
            y.rule = rule;
            if (rule == 0) {
                y.ztag = image_u64_bytes(image + my + 1);
                y.nonce_lo = image_u64_bytes(image + my + 9);
                y.nonce_hi = image_u64_bytes(image + my + 17);
            } else if (rule == 1) {
                const uint64_t pab = image_u64_bytes(image + my + 1);
                y.pa = (uint32_t)pab;
                y.pb = (uint32_t)(pab >> 32);
            }
            X.layers[lo + c + lane] = y;
        }
    }
}

// ---------------------------------------------------------------- parse: edges
// the u64 at byte address a of the image from three aligned dwords (two when a is 4-byte aligned)
__device__ __forceinline__ uint64_t image_u64(const uint32_t* __restrict__ img32, uint64_t a) {
    const uint64_t w = a >> 2;
    const uint32_t r = (uint32_t)a & 3u;
    const uint32_t d0 = img32[w], d1 = img32[w + 1], d2 = r ? img32[w + 2] : 0u;
    return (uint64_t)ct_funnel(d0, d1, r) | (uint64_t)ct_funnel(d1, d2, r) << 32;
}

template <bool WIDE>
__global__ __launch_bounds__(kImgBlock) void k_img_edges_parse(const uint32_t* __restrict__ img32, const uint64_t* __restrict__ pos,
                                                                const uint64_t* __restrict__ toff, const uint64_t* __restrict__ cE,
                                                                const uint64_t* __restrict__ oE, uint64_t n, pvac_ct_batch X,
                                                                ct_geom g, unsigned long long* __restrict__ ctl, uint64_t layer_cap,
                                                                uint64_t edge_cap, uint32_t* __restrict__ status) {
    if (!parse_go(ctl, layer_cap, edge_cap)) return;
    const uint64_t ntiles = ctl[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t sws = X.sigma ? X.sigma_words : 0u;
    const uint32_t pp = 3u + (WIDE ? sws / 2u : sws);   // output pieces per edge
    const uint64_t eb = g.eb();
    const uint64_t per = (ntiles + gridDim.x - 1) / gridDim.x;   // a run of consecutive tiles, as in the writer
    uint64_t t = blockIdx.x * per;
    const uint64_t t1 = t + per < ntiles ? t + per : ntiles;
    if (t >= t1) return;
    uint64_t i = tile_cipher(toff, n, t);
    for (; t < t1; ++t) {
        while (i + 1 < n && toff[i + 1] <= t) ++i;
        const uint64_t E = cE[i];
        const uint64_t ea = (t - toff[i]) * g.ept;
        const uint32_t ne = (uint32_t)(E - ea < g.ept ? E - ea : g.ept);
        const uint64_t bs = pos[i + 1] - (E - ea) * eb;
        const uint64_t slot = oE[i] + ea;
        for (uint32_t x = tid; x < ne * pp; x += kImgBlock) {
            const uint32_t e = x / pp, p = x - e * pp;
            const uint64_t rec = bs + (uint64_t)e * eb;
            if (p == 0) {
                X.meta[slot + e] = image_u64(img32, rec) & 0x00FFFFFFFFFFFFFFull;
            } else if (p == 1) {
                X.w_lo[slot + e] = image_u64(img32, rec + 8);
            } else if (p == 2) {
                X.w_hi[slot + e] = image_u64(img32, rec + 16);
                if (ct_image_u32(img32, rec + 24) != g.nbits) {
                    atomicAdd(&ctl[4], 1ull);
                    if (status) atomicMax(&status[i], 2u);
                }
            } else if (WIDE) {
                const uint32_t q = p - 3;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (2 * q < g.nw) {   // nw is even on this path: both words come from the image
                    const uint64_t a = rec + 28 + 16ull * q, w = a >> 2;
                    const uint32_t r = (uint32_t)a & 3u;
                    const uint32_t d0 = img32[w], d1 = img32[w + 1], d2 = img32[w + 2], d3 = img32[w + 3];
                    const uint32_t d4 = r ? img32[w + 4] : 0u;
                    v = make_uint4(ct_funnel(d0, d1, r), ct_funnel(d1, d2, r), ct_funnel(d2, d3, r), ct_funnel(d3, d4, r));
                }
                *(uint4*)(X.sigma + (slot + e) * sws + 2 * q) = v;
            } else {
                const uint32_t q = p - 3;
                X.sigma[(slot + e) * sws + q] = q < g.nw ? image_u64(img32, rec + 28 + 8ull * q) : 0ull;
            }
        }
    }
}

unsigned grid_for(uint64_t items, unsigned per_block) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace

hipError_t launch_ct_image_plan(const pvac_ct_batch& X, uint32_t nbits, uint64_t* sz, uint64_t* tcnt, uint64_t* scan_scratch,
                                unsigned long long* ctl, uint64_t* pos, hipStream_t st) {
    const ct_geom g = ct_geom_of(nbits);
    hipError_t e = hipMemsetAsync(ctl, 0, kCtImageCtlWords * 8, st);
    if (e != hipSuccess) return e;
    if (X.n) hipLaunchKernelGGL(k_img_sizes, dim3(grid_for(8 * X.n, kImgBlock)), dim3(kImgBlock), 0, st, X, g, sz, ctl);
    e = launch_exclusive_scan_u64(sz, X.n, scan_scratch, &ctl[0], st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_img_pos, dim3(grid_for(X.n + 1, kImgBlock)), dim3(kImgBlock), 0, st, X, g, sz, ctl, pos, tcnt);
    e = launch_exclusive_scan_u64(tcnt, X.n, scan_scratch, &ctl[1], st);
    return e == hipSuccess ? hipGetLastError() : e;
}

hipError_t launch_ct_image_write(const pvac_ct_batch& X, uint32_t nbits, const uint64_t* pos, const uint64_t* toff,
                                 uint64_t ntiles, uint32_t max_tile_edges, bool wide, int num_cus, uint8_t* image, hipStream_t st) {
    const ct_geom g = ct_geom_of(nbits);
    if (max_tile_edges > g.ept) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_img_heads, dim3((unsigned)(X.n + 1)), dim3(64), 0, st, X, pos, image);
    if (ntiles) {
        const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, (uint64_t)num_cus * 64);
        const size_t lds = 4 * (size_t)ct_image_lds_words(max_tile_edges, g);
        if (wide)
            hipLaunchKernelGGL(k_img_edges_write<true>, dim3(grid), dim3(kImgBlock), lds, st, X, g, pos, toff, ntiles, max_tile_edges,
                               image);
        else
            hipLaunchKernelGGL(k_img_edges_write<false>, dim3(grid), dim3(kImgBlock), lds, st, X, g, pos, toff, ntiles, max_tile_edges,
                               image);
    }
    return hipGetLastError();
}

hipError_t launch_ct_image_parse(const uint8_t* image, uint64_t len, const uint64_t* pos, uint64_t n, uint32_t nbits,
                                 const pvac_ct_batch& X, uint64_t layer_cap, uint64_t edge_cap, uint32_t* status, uint64_t* words,
                                 uint64_t* scan_scratch, unsigned long long* ctl, bool wide, int num_cus, hipStream_t st) {
    const ct_geom g = ct_geom_of(nbits);
    const uint32_t* img32 = (const uint32_t*)image;
    const uint64_t stride = n + 1;
    uint64_t *cL = words, *cE = words + stride, *oL = words + 2 * stride, *oE = words + 3 * stride, *tc = words + 4 * stride;
    hipError_t e = hipMemsetAsync(ctl, 0, kCtImageCtlWords * 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_img_validate, dim3(grid_for(n ? n : 1, kImgBlock)), dim3(kImgBlock), 0, st, img32, len, pos, n, g, status,
                       cL, cE, oL, oE, tc, ctl);
    e = launch_exclusive_scan2_u64(oL, oE, n, scan_scratch, &ctl[0], &ctl[1], st);
    if (e == hipSuccess) e = launch_exclusive_scan_u64(tc, n, scan_scratch, &ctl[2], st);
    if (e != hipSuccess || !n) return e;
    hipLaunchKernelGGL(k_img_layers_parse, dim3((unsigned)n), dim3(64), 0, st, image, pos, cL, cE, oL, oE, X, ctl, layer_cap, edge_cap);
    // the tile count stays on the device: edge_cap bounds it (every tile but a cipher's last is full)
    const uint64_t bound = n + edge_cap / g.ept;
    const unsigned grid = (unsigned)std::min<uint64_t>(bound, (uint64_t)num_cus * 64);
    if (wide)
        hipLaunchKernelGGL(k_img_edges_parse<true>, dim3(grid), dim3(kImgBlock), 0, st, img32, pos, tc, cE, oE, n, X, g, ctl, layer_cap,
                           edge_cap, status);
    else
        hipLaunchKernelGGL(k_img_edges_parse<false>, dim3(grid), dim3(kImgBlock), 0, st, img32, pos, tc, cE, oE, n, X, g, ctl, layer_cap,
                           edge_cap, status);
    return hipGetLastError();
}

}  // namespace pvhip
