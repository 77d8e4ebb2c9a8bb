// k_enc_wide.hip — the wide route of pvac_hip_enc_items on CDNA4: enc_fp_depth / enc_value_depth
// (reference ops/encrypt.hpp:162-258, 281-287) for noise plans beyond the 256 pre-merge edges per half
// that k_enc_items.hip holds (depth hints above 124 with the default Params; enc_text past 1,845
// bytes). The draws, the equations and the outputs are those of the narrow route, and the two agree
// byte for byte on every plan both can run (PVAC_ENC_WIDE_ALL). What differs is that nothing here is
// quadratic in npre and no index is a byte:
//   k_encw_replay   one lane per item walks its draws in the reference's order (a VALUE item: the mask,
//                   the second half, the first), notes every edge in its half's key table (enc_wide.hpp
//                   step 1: O(1) per edge), and runs the Fisher-Yates shuffle on 32-bit slots;
//   k_encw_order    one workgroup per half scans the 2 B keys of the table (ranks, segment starts) and
//                   places the edges: a stable counting sort, segments in creation order;
//   k_encw_delta    the last noise group's Delta = -(sum of the others), an order-exact fp_add chain,
//   k_encw_weights  once per half; then one thread per (half, group) with weights_entry's equations;
//   k_encw_finish   one wave per OUTPUT edge: the fp_add chain over its segment, the sigma rows of
//                   its contributors XORed with consecutive lanes on consecutive 16-byte chunks.
// The key tables live in global scratch (B may be 65,536: 512 KiB per half), not in LDS.
#include "common.hpp"
#include "enc_dev.hpp"
#include "enc_wide.hpp"

namespace pvhip {
namespace {

constexpr int kEWB = 64;     // replay, delta, weights: threads per workgroup
constexpr int kEWO = 256;    // order, finish: four waves

// what the replay keeps of a half in registers (half_requests reads ztag, nlo, nhi)
struct half_scalars {
    uint64_t nlo, nhi, ztag;
};

// One enc_fp_depth draw replay into the half's pre-edge slots at po (ops/encrypt.hpp:162-258; the
// draws of enc_dev.hpp::plan_half in the same order), noting every edge in tab; then shuffle_edges
// (:155-160) over the nout distinct keys. Returns nout.
__device__ uint32_t replay_half(const enc_wide_args& a, uint32_t Z2, uint32_t Z3, rstream& rs, uint64_t po, uint32_t* tab,
                                half_scalars& H) {
    const uint32_t B = a.B;
    uint32_t* key = a.key + po;
    uint64_t *salt = a.salt + po, *rlo = a.rlo + po, *rhi = a.rhi + po;
    uint32_t *occ = a.occ + po, *slot = a.slot + po;
    H.nlo = rs.next();
    H.nhi = rs.next();
    H.ztag = layer_ztag(a.canon, H.nlo, H.nhi);
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
        rlo[j] = r.lo;
        rhi[j] = r.hi;
    }
    rlo[7] = 0;
    rhi[7] = 0;
    uint32_t nout = 0;
    auto edge = [&](uint32_t e, uint32_t i, uint32_t s) {   // make_edge draws the salt (encrypt.hpp:150-153)
        const uint32_t k = i | (s << 16);
        key[e] = k;
        salt[e] = rs.next();
        const uint32_t o = wide_note(tab, k);
        occ[e] = o;
        nout += o == 0 ? 1u : 0u;
    };
    for (int j = 0; j < 8; ++j) edge(j, idx[j], ch[j]);
    uint32_t np = 8;
    for (uint32_t t = 0; t < Z2; ++t) {   // encrypt.hpp:212-229
        const uint32_t i = (uint32_t)(rs.next() % B);
        uint32_t j;
        do { j = (uint32_t)(rs.next() % B); } while (j == i && !rs.over);
        const uint32_t s1 = (uint32_t)(rs.next() & 1), s2 = s1 ^ 1;
        const fp ri = rand_fp_nonzero(rs);
        rlo[np] = ri.lo; rhi[np] = ri.hi; edge(np, i, s1); ++np;
        rlo[np] = 0; rhi[np] = 0; edge(np, j, s2); ++np;
    }
    for (uint32_t t = 0; t < Z3; ++t) {   // encrypt.hpp:231-252
        const uint32_t i = (uint32_t)(rs.next() % B);
        uint32_t j, k;
        do { j = (uint32_t)(rs.next() % B); } while (j == i && !rs.over);
        do { k = (uint32_t)(rs.next() % B); } while ((k == i || k == j) && !rs.over);
        const uint32_t s1 = (uint32_t)(rs.next() & 1), s2 = (uint32_t)(rs.next() & 1), s3 = (uint32_t)(rs.next() & 1);
        const fp fa = rand_fp_nonzero(rs), fb = rand_fp_nonzero(rs);
        rlo[np] = fa.lo; rhi[np] = fa.hi; edge(np, i, s1); ++np;
        rlo[np] = fb.lo; rhi[np] = fb.hi; edge(np, j, s2); ++np;
        rlo[np] = 0; rhi[np] = 0; edge(np, k, s3); ++np;
    }
    for (uint32_t g = 0; g < nout; ++g) slot[g] = g;
    for (uint32_t i = nout > 1 ? nout - 1 : 0; i > 0; --i) {
        const uint32_t j = (uint32_t)(rs.next() % (uint64_t)(i + 1));
        const uint32_t t = slot[i];
        slot[i] = slot[j];
        slot[j] = t;
    }
    return nout;
}

__global__ __launch_bounds__(kEWB) void k_encw_replay(enc_wide_args a, prf_request* req, pvac_ct_batch pre, pvac_ct_batch C,
                                                      uint32_t* status) {
    const uint64_t t = (uint64_t)blockIdx.x * kEWB + threadIdx.x;
    if (t >= a.n) return;
    const enc_item_rec it = a.recs[t];
    const uint32_t item = a.item[t];
    const uint32_t npre = 8 + 2 * it.Z2 + 3 * it.Z3;
    const uint32_t per_half = 3 * max(it.Z2 + it.Z3, 1u);
    rstream rs{a.rnd + it.rnd_off, it.rnd_cnt, 0, false};
    fp v[2] = {fp{it.v_lo, it.v_hi}, fp{0, 0}};
    if (it.halves == 2) {   // enc_value_depth: layer 0 = enc_fp_depth(v + mask), layer 1 = enc_fp_depth(-mask)
        const fp mask = rand_fp_nonzero(rs);
        v[0] = fp_add(fp{it.v_lo, 0}, mask);
        v[1] = fp_neg(mask);
    }
    const uint64_t pi = a.pre_base + t;
    pre.l_off[pi] = it.half_off;
    pre.l_cnt[pi] = it.halves;
    pre.e_off[pi] = it.pre_off;
    pre.e_cnt[pi] = (uint64_t)it.halves * npre;
    uint64_t out_edges = 0;
    // the second argument of combine_ciphers is evaluated (and draws) first
    for (int h = (int)it.halves - 1; h >= 0; --h) {
        const uint64_t po = it.pre_off + (uint64_t)h * npre;
        half_scalars H;
        const uint32_t nout = replay_half(a, it.Z2, it.Z3, rs, po, a.tab + (2 * t + h) * 2ull * a.B, H);
        const uint64_t ro = it.req_off + (uint64_t)h * per_half;
        half_requests(it.Z2, it.Z3, H, req + ro);
        a.hdr[it.half_off + h] = enc_half_hdr{H.nlo, H.nhi, H.ztag, v[h].lo, v[h].hi, po, ro, npre, nout, it.Z2, it.Z3};
        pvac_layer y{};
        y.ztag = H.ztag;
        y.nonce_lo = H.nlo;
        y.nonce_hi = H.nhi;
        pre.layers[it.half_off + h] = y;
        C.layers[it.half_off + h] = y;
        for (uint32_t e = 0; e < npre; ++e) pre.meta[po + e] = make_meta((uint32_t)h, a.key[po + e] & 0xFFFFu, a.key[po + e] >> 16);
        out_edges += nout;
    }
    C.l_off[item] = a.base_l + it.half_off;
    C.l_cnt[item] = it.halves;
    C.e_off[item] = a.base_e + it.pre_off;
    C.e_cnt[item] = out_edges;
    status[item] = rs.over ? 1u : 0u;
}

// blockIdx.x = 2 t + h. Two workgroup scans (common.hpp, DPP wave scans) per 256 keys: a key's rank and
// its segment start.
__global__ __launch_bounds__(kEWO) void k_encw_order(enc_wide_args a) {
    const uint64_t t = blockIdx.x >> 1;
    const uint32_t h = blockIdx.x & 1;
    const enc_item_rec& it = a.recs[t];
    if (h >= it.halves) return;
    const enc_half_hdr& H = a.hdr[it.half_off + h];
    const uint64_t po = H.pre_off;
    const uint32_t npre = H.npre, keys = 2 * a.B;
    uint32_t* tab = a.tab + (uint64_t)blockIdx.x * keys;
    const int tid = threadIdx.x;
    __shared__ uint32_t part[kEWO / 64];
    uint32_t rank0 = 0, start0 = 0;   // present keys and edges below this step's keys
    for (uint32_t base = 0; base < keys; base += kEWO) {
        const uint32_t k = base + tid;
        const uint32_t cnt = k < keys ? tab[k] : 0;
        uint32_t present, edges;
        const uint32_t rank = block_exclusive_scan<kEWO>(cnt ? 1u : 0u, part, present);
        const uint32_t start = block_exclusive_scan<kEWO>(cnt, part, edges);
        if (cnt) wide_place_key(tab, a.gstart + po, k, rank0 + rank, start0 + start);
        rank0 += present;
        start0 += edges;
    }
    __syncthreads();   // the table's starts before the placement reads them
    for (uint32_t e = tid; e < npre; e += kEWO) wide_place_edge(tab, a.key + po, a.occ + po, a.ord + po, e);
}

__device__ __forceinline__ fp prod3_at(const uint64_t* c, uint32_t q) {
    return fp_mul(fp_mul(fp{c[2 * q], c[2 * q + 1]}, fp{c[2 * q + 2], c[2 * q + 3]}), fp{c[2 * q + 4], c[2 * q + 5]});
}

// one thread per half of the sub-batch's wide items: Delta of the last group (encrypt.hpp:205-210);
// fp_add does not canonicalise, so the chain runs in group order
__global__ __launch_bounds__(kEWB) void k_encw_delta(enc_wide_args a, const uint64_t* cores) {
    const uint64_t x = (uint64_t)blockIdx.x * kEWB + threadIdx.x;
    if (x >= 2 * a.n) return;
    const enc_item_rec& it = a.recs[x >> 1];
    const uint32_t h = (uint32_t)(x & 1);
    if (h >= it.halves) return;
    const uint64_t half = it.half_off + h;
    const enc_half_hdr& H = a.hdr[half];
    const uint32_t G = H.Z2 + H.Z3;
    const uint64_t* c = cores + 2 * H.req_off;
    fp dacc{0, 0};
    for (uint32_t q = 0; q + 1 < G; ++q) dacc = fp_add(dacc, prod3_at(c, 3 + 3 * q));
    const fp D = fp_neg(dacc);
    a.dlast[2 * half] = D.lo;
    a.dlast[2 * half + 1] = D.hi;
}

// one (half, group) of the equations (encrypt.hpp:184-252) and the weights w = r R of its edges:
// k_enc_items.hip's weights_entry with the last group's Delta read, not recomputed
__global__ __launch_bounds__(kEWB) void k_encw_weights(enc_wide_args a, const uint64_t* cores, pvac_ct_batch pre) {
    const uint64_t t = (uint64_t)blockIdx.x * kEWB + threadIdx.x;
    if (t >= a.n_work) return;
    const uint64_t half = a.work[t] >> 32;
    const uint32_t grp = (uint32_t)a.work[t];
    const enc_half_hdr& H = a.hdr[half];
    const uint32_t Z2 = H.Z2, G = H.Z2 + H.Z3;
    const uint64_t* c = cores + 2 * H.req_off;
    const fp R = prod3_at(c, 0);   // prf_R (lpn.hpp:263-268)
    const uint64_t po = H.pre_off;
    auto rr = [&](uint32_t e) { return fp{a.rlo[po + e], a.rhi[po + e]}; };
    auto idx = [&](uint32_t e) { return a.key[po + e] & 0xFFFFu; };
    auto chn = [&](uint32_t e) { return a.key[po + e] >> 16; };
    auto put = [&](uint32_t e, const fp& r) {
        const fp w = fp_mul(r, R);
        pre.w_lo[po + e] = w.lo;
        pre.w_hi[po + e] = w.hi;
    };
    if (grp == 0) {   // signal: the last coefficient solves sum(+/- r_j g^idx_j) = v
        fp sumg{0, 0};
        for (uint32_t j = 0; j < 7; ++j) {
            const fp r = rr(j);
            const fp term = fp_mul(r, powg_at(a.powg, idx(j)));
            sumg = chn(j) == 0 ? fp_add(sumg, term) : fp_sub(sumg, term);
            put(j, r);
        }
        const fp rl = fp_mul(fp_sub(fp{H.vlo, H.vhi}, sumg), fp_inv(powg_at(a.powg, idx(7))));
        put(7, chn(7) == 0 ? rl : fp_neg(rl));
        return;
    }
    const uint32_t g = grp - 1;
    const fp D = G - g <= 1 ? fp{a.dlast[2 * half], a.dlast[2 * half + 1]} : prod3_at(c, 3 + 3 * g);   // prf_R_noise
    if (g < Z2) {   // encrypt.hpp:212-229
        const uint32_t e = 8 + 2 * g;
        const fp Dp = chn(e) == 0 ? D : fp_neg(D);
        const fp ri = rr(e);
        const fp rj = fp_mul(fp_sub(fp_mul(ri, powg_at(a.powg, idx(e))), Dp), fp_inv(powg_at(a.powg, idx(e + 1))));
        put(e, ri);
        put(e + 1, rj);
    } else {        // encrypt.hpp:231-252
        const uint32_t e = 8 + 2 * Z2 + 3 * (g - Z2);
        const fp fa = rr(e), fb = rr(e + 1);
        fp t1 = fp_mul(fa, powg_at(a.powg, idx(e)));
        fp t2 = fp_mul(fb, powg_at(a.powg, idx(e + 1)));
        if (chn(e)) t1 = fp_neg(t1);
        if (chn(e + 1)) t2 = fp_neg(t2);
        const fp gk = chn(e + 2) == 0 ? powg_at(a.powg, idx(e + 2)) : fp_neg(powg_at(a.powg, idx(e + 2)));
        const fp cc = fp_mul(fp_sub(D, fp_add(t1, t2)), fp_inv(gk));
        put(e, fa);
        put(e + 1, fb);
        put(e + 2, cc);
    }
}

// A workgroup is dealt kEncWideFinChunk output slots of one half, a wave takes every fourth. Per output
// edge: compact_edges' fp_add chain from 0 over the segment in creation order and the sigma XOR
// (encrypt.hpp:45-58). The contributors' weights are loaded 64 at a time, one per lane, and chained
// through shuffles by every lane alike. WIDE16: sigma rows are 16-byte aligned and an even number of
// words, so consecutive lanes take consecutive 16-byte chunks.
template <bool WIDE16>
__global__ __launch_bounds__(kEWO) void k_encw_finish(enc_wide_args a, pvac_ct_batch pre, pvac_ct_batch C, uint32_t* status) {
    const uint64_t word = a.fin[blockIdx.x];
    const uint64_t half = word >> 32;
    const uint32_t s0 = (uint32_t)word;
    const enc_half_hdr& H = a.hdr[half];
    const uint32_t hi = a.half_item[half], h = hi & 1, item = hi >> 1;
    const uint32_t npre = H.npre, nout = H.nout;
    const uint64_t po = H.pre_off;
    // output slots of the item: the first half's merged edges, then the second's
    const uint64_t dst0 = po - (uint64_t)h * npre + (h ? a.hdr[half - 1].nout : 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t sw = C.sigma_words;
    const bool sig = pre.sigma && C.sigma;
    const uint32_t* ord = a.ord + po;
    for (uint32_t s = s0 + wave; s < s0 + kEncWideFinChunk && s < nout; s += kEWO / 64) {
        uint32_t b, e;
        wide_segment(a.gstart + po, nout, npre, a.slot[po + s], b, e);
        fp w{0, 0};
        for (uint32_t q0 = b; q0 < e; q0 += 64) {
            const uint32_t m = min(e - q0, 64u);
            uint64_t wl = 0, wh = 0;
            if ((uint32_t)lane < m) {
                const uint32_t pe = ord[q0 + lane];
                wl = pre.w_lo[po + pe];
                wh = pre.w_hi[po + pe];
            }
            for (uint32_t q = 0; q < m; ++q) w = fp_add(w, fp{__shfl(wl, (int)q, 64), __shfl(wh, (int)q, 64)});
        }
        const uint32_t key = a.key[po + ord[b]];
        const uint64_t dst = dst0 + s;
        uint64_t any = 0;
        if (sig) {
            if (WIDE16) {
                for (uint32_t cidx = lane; cidx < sw / 2; cidx += 64) {
                    ulonglong2 x = make_ulonglong2(0, 0);
                    for (uint32_t q = b; q < e; ++q) {
                        const ulonglong2 r = ((const ulonglong2*)(pre.sigma + (po + ord[q]) * (uint64_t)pre.sigma_words))[cidx];
                        x.x ^= r.x;
                        x.y ^= r.y;
                    }
                    ((ulonglong2*)(C.sigma + dst * sw))[cidx] = x;
                    any |= x.x | x.y;
                }
            } else {
                for (uint32_t wd = lane; wd < sw; wd += 64) {
                    uint64_t x = 0;
                    for (uint32_t q = b; q < e; ++q) x ^= pre.sigma[(po + ord[q]) * (uint64_t)pre.sigma_words + wd];
                    C.sigma[dst * sw + wd] = x;
                    any |= x;
                }
            }
        }
        const bool sig_nz = __ballot(any != 0) != 0;
        if (lane == 0) {
            C.meta[dst] = make_meta(h, key & 0xFFFFu, key >> 16);
            C.w_lo[dst] = w.lo;
            C.w_hi[dst] = w.hi;
            if (!(w.lo | w.hi) && !sig_nz) atomicCAS(&status[item], 0u, 2u);   // a merged group vanished
        }
    }
}

__global__ __launch_bounds__(kEWB) void k_enc_scatter_index(uint64_t n, const uint32_t* nid, pvac_ct_batch tmp,
                                                            const uint32_t* tmp_status, uint64_t base_l, uint64_t base_e,
                                                            pvac_ct_batch C, uint32_t* status) {
    const uint64_t t = (uint64_t)blockIdx.x * kEWB + threadIdx.x;
    if (t >= n) return;
    const uint32_t i = nid[t];
    C.l_off[i] = tmp.l_off[t] + base_l;
    C.l_cnt[i] = tmp.l_cnt[t];
    C.e_off[i] = tmp.e_off[t] + base_e;
    C.e_cnt[i] = tmp.e_cnt[t];
    status[i] = tmp_status[t];
}

bool grid_ok(uint64_t blocks) { return blocks <= 0x7FFFFFFFull; }

}  // namespace

hipError_t launch_enc_wide_replay(const enc_wide_args& a, prf_request* req, pvac_ct_batch& pre, pvac_ct_batch& C,
                                  uint32_t* status, hipStream_t st) {
    if (!a.n) return hipSuccess;
    const uint64_t blocks = (a.n + kEWB - 1) / kEWB;
    if (a.B == 0 || a.B > 65536 || !grid_ok(blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_encw_replay, dim3((unsigned)blocks), dim3(kEWB), 0, st, a, req, pre, C, status);
    return hipGetLastError();
}

hipError_t launch_enc_wide_order(const enc_wide_args& a, hipStream_t st) {
    if (!a.n) return hipSuccess;
    if (!grid_ok(2 * a.n)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_encw_order, dim3((unsigned)(2 * a.n)), dim3(kEWO), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_enc_wide_weights(const enc_wide_args& a, const uint64_t* cores, pvac_ct_batch& pre, hipStream_t st) {
    if (!a.n) return hipSuccess;
    const uint64_t bd = (2 * a.n + kEWB - 1) / kEWB, bw = (a.n_work + kEWB - 1) / kEWB;
    if (!grid_ok(bd) || !grid_ok(bw)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_encw_delta, dim3((unsigned)bd), dim3(kEWB), 0, st, a, cores);
    if (bw) hipLaunchKernelGGL(k_encw_weights, dim3((unsigned)bw), dim3(kEWB), 0, st, a, cores, pre);
    return hipGetLastError();
}

hipError_t launch_enc_wide_finish(const enc_wide_args& a, const pvac_ct_batch& pre, pvac_ct_batch& C, uint32_t* status,
                                  hipStream_t st) {
    if (!a.n || !a.n_fin) return hipSuccess;
    if (!grid_ok(a.n_fin)) return hipErrorInvalidValue;
    const bool sig = pre.sigma && C.sigma;
    const bool wide16 = sig && C.sigma_words % 2 == 0 && pre.sigma_words % 2 == 0 && (uintptr_t)C.sigma % 16 == 0 &&
                        (uintptr_t)pre.sigma % 16 == 0;
    if (wide16)
        hipLaunchKernelGGL(k_encw_finish<true>, dim3((unsigned)a.n_fin), dim3(kEWO), 0, st, a, pre, C, status);
    else
        hipLaunchKernelGGL(k_encw_finish<false>, dim3((unsigned)a.n_fin), dim3(kEWO), 0, st, a, pre, C, status);
    return hipGetLastError();
}

hipError_t launch_enc_scatter_index(uint64_t n, const uint32_t* nid, const pvac_ct_batch& tmp, const uint32_t* tmp_status,
                                    uint64_t base_l, uint64_t base_e, pvac_ct_batch& C, uint32_t* status, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + kEWB - 1) / kEWB;
    if (!grid_ok(blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_enc_scatter_index, dim3((unsigned)blocks), dim3(kEWB), 0, st, n, nid, tmp, tmp_status, base_l, base_e, C,
                       status);
    return hipGetLastError();
}

}  // namespace pvhip
