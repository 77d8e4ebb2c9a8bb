// k_enc_items.hip — a ragged batch of encryptions on CDNA4: every item is a bare enc_fp_depth
// (reference ops/encrypt.hpp:162-258: one BASE layer, a 127-bit plaintext as given) or the masked
// enc_value_depth form (:281-287, two layers), with its own depth hint — so its own noise plan
// (Z2, Z3) — and its own draw segment. enc_text (utils/text.hpp:39-61) is one such batch per message:
// the length as a value item, then one bare item per 15-byte block with hints 2, 3, ...
//
// The draw order, the merge groups and the equations are those of k_enc.hip (the replay itself is
// shared, enc_dev.hpp). What differs is the layout: per-half scratch is structure-of-arrays over the
// halves' pre-merge edge slots (enc_items_args), since plans from 8 to 255 pre-edges share a launch;
// k_enc_items_plan deals the items through a host-built permutation, largest plan first (its
// grouping is O(npre^2), and a wave costs its heaviest lane); and k_enc_items_weights runs one thread
// per (half, group) instead of per half: every group costs an fp_inv (~137 fp_mul), a hint-124 half
// has 105 of them, and a message of a few dozen blocks would otherwise wait for that one chain.
#include "common.hpp"
#include "enc_dev.hpp"

namespace pvhip {
namespace {

constexpr int kEIB = 64;

// plan_half's view of one half: the scalars live in registers until the header is written
struct half_soa {
    uint64_t nlo, nhi, ztag, vlo, vhi;
    uint32_t npre, nout;
    uint32_t* key;
    uint64_t *salt, *rlo, *rhi;
    uint8_t *grp, *slot;
};

__device__ half_soa half_at(const enc_items_args& a, uint64_t pre_off) {
    half_soa H{};
    H.key = a.key + pre_off;
    H.salt = a.salt + pre_off;
    H.rlo = a.rlo + pre_off;
    H.rhi = a.rhi + pre_off;
    H.grp = a.grp + pre_off;
    H.slot = a.slot + pre_off;
    return H;
}

__global__ __launch_bounds__(kEIB) void k_enc_items_plan(enc_items_args a, prf_request* req, pvac_ct_batch pre,
                                                         uint32_t* status) {
    const uint64_t t = (uint64_t)blockIdx.x * kEIB + threadIdx.x;
    if (t >= a.n) return;
    const uint64_t i = a.perm[t];
    const enc_item_rec it = a.recs[i];
    const uint32_t npre = 8 + 2 * it.Z2 + 3 * it.Z3;
    const uint32_t per_half = 3 * max(it.Z2 + it.Z3, 1u);
    rstream rs{a.rnd + it.rnd_off, it.rnd_cnt, 0, false};
    fp v[2] = {fp{it.v_lo, it.v_hi}, fp{0, 0}};
    if (it.halves == 2) {   // enc_value_depth: layer 0 = enc_fp_depth(v + mask), layer 1 = enc_fp_depth(-mask)
        const fp mask = rand_fp_nonzero(rs);
        v[0] = fp_add(fp{it.v_lo, 0}, mask);
        v[1] = fp_neg(mask);
    }
    pre.l_off[i] = it.half_off;
    pre.l_cnt[i] = it.halves;
    pre.e_off[i] = it.pre_off;
    pre.e_cnt[i] = (uint64_t)it.halves * npre;
    // the second argument of combine_ciphers is evaluated (and draws) first
    for (int h = (int)it.halves - 1; h >= 0; --h) {
        const uint64_t po = it.pre_off + (uint64_t)h * npre;
        half_soa H = half_at(a, po);
        plan_half(a.canon, a.B, it.Z2, it.Z3, rs, v[h], H);
        const uint64_t ro = it.req_off + (uint64_t)h * per_half;
        half_requests(it.Z2, it.Z3, H, req + ro);
        a.hdr[it.half_off + h] = enc_half_hdr{H.nlo, H.nhi, H.ztag, H.vlo, H.vhi, po, ro, H.npre, H.nout, it.Z2, it.Z3};
        pvac_layer y{};
        y.ztag = H.ztag;
        y.nonce_lo = H.nlo;
        y.nonce_hi = H.nhi;
        pre.layers[it.half_off + h] = y;
        for (uint32_t e = 0; e < npre; ++e) pre.meta[po + e] = make_meta((uint32_t)h, H.key[e] & 0xFFFFu, H.key[e] >> 16);
    }
    status[i] = rs.over ? 1u : 0u;
}

// one (half, group) of the equations (encrypt.hpp:184-252) and the weights w = r R of its edges
__device__ void weights_entry(const enc_items_args& a, const uint64_t* cores, const pvac_ct_batch& pre, uint64_t half,
                              uint32_t grp) {
    const enc_half_hdr& H = a.hdr[half];
    const uint32_t Z2 = H.Z2, G = H.Z2 + H.Z3;
    const uint64_t* c = cores + 2 * H.req_off;
    auto core = [&](uint32_t q) { return fp{c[2 * q], c[2 * q + 1]}; };
    auto prod3 = [&](uint32_t q) { return fp_mul(fp_mul(core(q), core(q + 1)), core(q + 2)); };
    const fp R = prod3(0);   // prf_R (lpn.hpp:263-268)
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
    // noise group g: Delta_g = prf_noise_delta for all but the last, which takes -(their sum): the
    // fp_add chain in group order (fp_add does not canonicalise, so the order is part of the result)
    const uint32_t g = grp - 1;
    fp D;
    if (G - g <= 1) {
        fp dacc{0, 0};
        for (uint32_t q = 0; q + 1 < G; ++q) dacc = fp_add(dacc, prod3(3 + 3 * q));
        D = fp_neg(dacc);
    } else {
        D = prod3(3 + 3 * g);   // prf_R_noise
    }
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

#ifndef PVAC_ENC_ITEMS_PER_HALF
__global__ __launch_bounds__(kEIB) void k_enc_items_weights(enc_items_args a, const uint64_t* cores, pvac_ct_batch pre) {
    const uint64_t t = (uint64_t)blockIdx.x * kEIB + threadIdx.x;
    if (t >= a.n_work) return;
    const uint64_t w = a.work[t];
    weights_entry(a, cores, pre, w >> 16, (uint32_t)(w & 0xFFFFu));
}
#else
// measurement variant (make variant VFLAGS=-DPVAC_ENC_ITEMS_PER_HALF): one thread per half runs its groups in turn
__global__ __launch_bounds__(kEIB) void k_enc_items_weights(enc_items_args a, const uint64_t* cores, pvac_ct_batch pre) {
    const uint64_t t = (uint64_t)blockIdx.x * kEIB + threadIdx.x;
    if (t >= a.n_halves) return;
    const uint32_t G = a.hdr[t].Z2 + a.hdr[t].Z3;
    for (uint32_t grp = 0; grp <= G; ++grp) weights_entry(a, cores, pre, t, grp);
}
#endif

// one wave per item: merged groups in shuffled order; lanes XOR sigma words
__global__ __launch_bounds__(kEIB) void k_enc_items_finish(enc_items_args a, pvac_ct_batch pre, pvac_ct_batch C,
                                                           uint32_t* status) {
    const uint64_t i = blockIdx.x;
    if (i >= a.n) return;
    const int lane = threadIdx.x;
    const uint64_t lo = a.recs[i].half_off, eo = a.recs[i].pre_off;
    const uint32_t halves = a.recs[i].halves;
    uint32_t pos = 0;
    bool vanished = false;
    for (uint32_t h = 0; h < halves; ++h) {
        const enc_half_hdr& H = a.hdr[lo + h];
        const uint64_t po = H.pre_off;
        if (lane == 0) {
            pvac_layer y{};
            y.ztag = H.ztag;
            y.nonce_lo = H.nlo;
            y.nonce_hi = H.nhi;
            C.layers[lo + h] = y;
        }
        for (uint32_t s = 0; s < H.nout; ++s) {
            const uint32_t g = a.slot[po + s];
            fp w{0, 0};
            uint32_t key = 0;
            uint64_t any = 0;
            // compact_edges: fp_add chain in creation order from 0, sigma XOR (encrypt.hpp:45-58)
            for (uint32_t e = 0; e < H.npre; ++e) {
                if (a.grp[po + e] != g) continue;
                w = fp_add(w, fp{pre.w_lo[po + e], pre.w_hi[po + e]});
                key = a.key[po + e];
            }
            const uint64_t dst = eo + pos + s;
            if (pre.sigma && C.sigma) {
                for (uint32_t wd = lane; wd < C.sigma_words; wd += 64) {
                    uint64_t x = 0;
                    for (uint32_t e = 0; e < H.npre; ++e)
                        if (a.grp[po + e] == g) x ^= pre.sigma[(po + e) * pre.sigma_words + wd];
                    C.sigma[dst * C.sigma_words + wd] = x;
                    any |= x;
                }
            }
            const bool sig_nz = __ballot(any != 0) != 0;
            vanished |= !(w.lo | w.hi) && !sig_nz;
            if (lane == 0) {
                C.meta[dst] = make_meta(h, key & 0xFFFFu, key >> 16);
                C.w_lo[dst] = w.lo;
                C.w_hi[dst] = w.hi;
            }
        }
        pos += H.nout;
    }
    if (lane == 0) {
        C.l_off[i] = lo;
        C.l_cnt[i] = halves;
        C.e_off[i] = eo;
        C.e_cnt[i] = pos;
        if (vanished && status[i] == 0) status[i] = 2;
    }
}

}  // namespace

hipError_t launch_enc_items_plan(const enc_items_args& a, prf_request* req, pvac_ct_batch& pre, uint32_t* status,
                                 hipStream_t st) {
    if (!a.n) return hipSuccess;
    if (a.B == 0 || a.B > 65536 || a.n > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_enc_items_plan, dim3((unsigned)((a.n + kEIB - 1) / kEIB)), dim3(kEIB), 0, st, a, req, pre, status);
    return hipGetLastError();
}

hipError_t launch_enc_items_weights(const enc_items_args& a, const uint64_t* cores, pvac_ct_batch& pre, hipStream_t st) {
    if (!a.n) return hipSuccess;
#ifndef PVAC_ENC_ITEMS_PER_HALF
    const uint64_t threads = a.n_work;
#else
    const uint64_t threads = a.n_halves;
#endif
    if ((threads + kEIB - 1) / kEIB > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_enc_items_weights, dim3((unsigned)((threads + kEIB - 1) / kEIB)), dim3(kEIB), 0, st, a, cores, pre);
    return hipGetLastError();
}

hipError_t launch_enc_items_finish(const enc_items_args& a, const pvac_ct_batch& pre, pvac_ct_batch& C, uint32_t* status,
                                   hipStream_t st) {
    if (!a.n) return hipSuccess;
    if (a.n > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_enc_items_finish, dim3((unsigned)a.n), dim3(kEIB), 0, st, a, pre, C, status);
    return hipGetLastError();
}

}  // namespace pvhip
