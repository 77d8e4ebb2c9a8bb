// rt_keys.cpp — what hangs on the keys: H and its digest, sigma_batch, the secret key and the LPN
// PRF, enc_value, base_R and dec_value.
#include <cmath>

#include "ctx.hpp"
#include "enc_wide.hpp"
#include "sha256.hpp"

using namespace pvhip;

extern "C" {

// ---------------------------------------------------------------- sigma / H
int pvac_hip_ctx_set_H(pvac_hip_ctx* c, const uint64_t* H, uint32_t n_cols, uint32_t wpc) try {
    if (!c || !H) return PVAC_EINVAL;
    if (n_cols != c->prm.n_bits || wpc != (c->prm.m_bits + 63) / 64) return fail(c, PVAC_EINVAL, "set_H: shape");
    const int rc = hip_fail(c, sigma_tables_from_dense(c->H, c->prm, H, c->stream), "set_H");
    if (rc) return rc;
    ++c->H_gen;
    // H_digest = SHA-256("H|v2" || le64 m || le64 n || le64 wt || column bytes) (matrix.hpp:218-250)
    const size_t colbytes = (c->prm.m_bits + 7) / 8;
    std::vector<uint8_t> msg(28 + (size_t)n_cols * colbytes);
    std::memcpy(msg.data(), "H|v2", 4);
    const uint64_t hdr[3] = {c->prm.m_bits, c->prm.n_bits, c->prm.h_col_wt};
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 8; ++i) msg[4 + 8 * k + i] = (uint8_t)(hdr[k] >> (8 * i));
    for (uint32_t col = 0; col < n_cols; ++col)
        for (size_t b = 0; b < colbytes; ++b)
            msg[28 + (size_t)col * colbytes + b] = (uint8_t)(H[(size_t)col * wpc + b / 8] >> (8 * (b % 8)));
    sha256_host(msg.data(), msg.size(), c->H_digest);
    c->have_digest = true;
    return PVAC_OK;
} catch (...) { return caught(c, "set_H"); }

int pvac_hip_ctx_gen_H(pvac_hip_ctx* c, uint8_t digest[32]) try {
    if (!c) return PVAC_EINVAL;
    scoped_timer t(c, "gen_H");
    uint8_t d[32];
    const int rc = hip_fail(c, sigma_tables_generate(c->H, c->prm, d, c->stream), "gen_H");
    if (rc) return rc;
    ++c->H_gen;
    std::memcpy(c->H_digest, d, 32);
    c->have_digest = true;
    if (digest) std::memcpy(digest, d, 32);
    return PVAC_OK;
} catch (...) { return caught(c, "gen_H"); }

int pvac_hip_sigma_batch(pvac_hip_ctx* c, pvac_ct_batch* X, const uint64_t* salts) try {
    if (!c || !batch_ok(X) || !salts || !X->sigma) return PVAC_EINVAL;
    if (!c->H.ready) return fail(c, PVAC_EINVAL, "sigma_batch: H not set");
    scoped_timer t(c, "sigma");
    return hip_fail(c, launch_sigma(c->H, c->prm, *X, salts, nullptr, c->num_cus, c->stream), "sigma");
} catch (...) { return caught(c, "sigma_batch"); }

// ---------------------------------------------------------------- LPN PRF
int pvac_hip_ctx_set_secret(pvac_hip_ctx* c, const uint64_t prf_k[4], const uint64_t* lpn_s_host, uint32_t lpn_n,
                            uint32_t lpn_t, uint32_t tau_num, uint32_t tau_den) try {
    if (!c || !prf_k || !lpn_s_host) return fail(c, PVAC_EINVAL, "set_secret: arguments");
    const uint32_t words = (lpn_n + 63) / 64;
    if (lpn_n == 0 || words > 64 || tau_den == 0 || tau_num > tau_den)
        return fail(c, PVAC_EINVAL, "set_secret: lpn_n must be in [1, 4096], 0 <= tau_num <= tau_den, tau_den > 0");
    if (lpn_t < 127) return fail(c, PVAC_ENOSYS, "set_secret: lpn_t < 127 not supported");
    c->prf.lpn_s.release();
    c->prf.have_secret = false;
    hipError_t e = c->prf.lpn_s.grow(64, 64);
    if (e == hipSuccess) e = hipMemset(c->prf.lpn_s.get(), 0, 64 * 8);
    if (e == hipSuccess) e = hipMemcpy(c->prf.lpn_s.get(), lpn_s_host, (size_t)words * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(c, e, "set_secret");
    std::memcpy(c->prf.k, prf_k, 32);
    c->prf.lpn_words = words;
    c->prf.lpn_t = lpn_t;
    c->prf.tau_num = tau_num;
    c->prf.tau_den = tau_den;
    c->prf.have_secret = true;
    return PVAC_OK;
} catch (...) { return caught(c, "set_secret"); }

int pvac_hip_ctx_set_H_digest(pvac_hip_ctx* c, const uint8_t digest[32]) {
    if (!c || !digest) return PVAC_EINVAL;
    std::memcpy(c->H_digest, digest, 32);
    c->have_digest = true;
    return PVAC_OK;
}

namespace {

uint64_t fnv1a(const char* d) {   // lpn.hpp:150-157
    uint64_t h = 0xcbf29ce484222325ull;
    for (const char* p = d; *p; ++p) { h ^= (uint8_t)*p; h *= 0x100000001b3ull; }
    return h;
}

// constants of the key derivation (lpn.hpp:159-186); the first message block is fixed per key
int prf_setup(pvac_hip_ctx* c, prf_consts& k) {
    if (!c->prf.have_secret) return fail(c, PVAC_EINVAL, "prf: secret key not set (pvac_hip_ctx_set_secret)");
    if (!c->have_digest) return fail(c, PVAC_EINVAL, "prf: H_digest unknown (gen_H, set_H or set_H_digest)");
    if (!c->prf.aes_tables) {
        hipError_t e = prf_upload_tables(c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "prf tables");
        c->prf.aes_tables = true;
    }
    uint8_t m[64];
    for (int i = 0; i < 4; ++i)
        for (int b = 0; b < 8; ++b) m[8 * i + b] = (uint8_t)(c->prf.k[i] >> (8 * b));
    for (int b = 0; b < 8; ++b) m[32 + b] = (uint8_t)(c->prm.canon_tag >> (8 * b));
    std::memcpy(m + 40, c->H_digest, 24);
    uint32_t w[16];
    for (int i = 0; i < 16; ++i)
        w[i] = (uint32_t)m[4 * i] << 24 | (uint32_t)m[4 * i + 1] << 16 | (uint32_t)m[4 * i + 2] << 8 | m[4 * i + 3];
    sha_state st;
    sha_init(st);
    sha_compress(st, w);
    std::memcpy(k.mid, st.h, 32);
    uint64_t tail = 0;
    for (int b = 0; b < 8; ++b) tail |= (uint64_t)c->H_digest[24 + b] << (8 * b);
    k.hd_tail = tail;
    static const char* const doms[6] = {"pvac.prf.r.1", "pvac.prf.r.2", "pvac.prf.r.3",
                                        "pvac.prf.noise.1", "pvac.prf.noise.2", "pvac.prf.noise.3"};
    for (int d = 0; d < 6; ++d) k.dom_hash[d] = fnv1a(doms[d]);
    k.toep_hash = fnv1a("pvac.dom.toeplitz");
    k.s_bits = c->prf.lpn_s.get();
    k.s_words = c->prf.lpn_words;
    k.tau_num = c->prf.tau_num;
    k.tau_den = c->prf.tau_den;
    return PVAC_OK;
}

int ensure_prf_scratch(pvac_hip_ctx* c, uint64_t cores) {
    int rc = hip_fail(c, c->prf.req.grow_floor(cores * prf_request_bytes()), "alloc prf requests");
    if (rc) return rc;
    return hip_fail(c, c->prf.core.grow_floor(2 * cores), "alloc prf cores");
}

}  // namespace

int pvac_hip_prf(pvac_hip_ctx* c, int kind, size_t n, const uint64_t* seeds, uint64_t* out) try {
    if (!c || kind < 0 || kind > 7 || (n && (!seeds || !out))) return fail(c, PVAC_EINVAL, "prf: arguments");
    if (!n) return PVAC_OK;
    prf_consts k{};
    int rc = prf_setup(c, k);
    if (rc) return rc;
    rc = ensure_prf_scratch(c, 3 * (uint64_t)n);
    if (rc) return rc;
    scoped_timer t(c, "prf");
    return hip_fail(c, launch_prf(k, kind, seeds, n, c->prf.req.get(), c->prf.core.get(), out, c->stream), "prf");
} catch (...) { return caught(c, "prf"); }

// ---------------------------------------------------------------- enc_value
namespace {
// ops/encrypt.hpp:16-27 with the context's noise Params (the reference's defaults: noise_entropy_bits
// 120, tuple2_fraction 0.55, depth_slope_bits 16; pvac_hip_ctx_set_noise); enc_value uses depth_hint 0
void plan_noise(const pvac_hip_ctx* c, int depth, uint32_t& z2, uint32_t& z3) {
    const uint32_t B = c->prm.B;
    const double budget = c->prf.noise_bits + c->prf.noise_slope * std::max(0, depth);
    const double per2 = 2.0 * std::log2((double)B), per3 = 3.0 * std::log2((double)B);
    int a = std::max(0, (int)std::floor((budget * c->prf.noise_t2) / std::max(1e-6, per2)));
    int b = std::max(0, (int)std::floor((budget * (1.0 - c->prf.noise_t2)) / std::max(1e-6, per3)));
    if (a + b == 1) { if (b > 0) ++b; else ++a; }
    z2 = (uint32_t)a;
    z3 = (uint32_t)b;
}
// a plan above the context's limit (pvac_hip_ctx_set_enc_plan_limit) is refused before anything happens
bool plan_over(const pvac_hip_ctx* c, uint32_t z2, uint32_t z3) { return enc_npre(z2, z3) > c->prf.enc_plan_limit; }
int plan_refused(pvac_hip_ctx* c, const char* who) {   // PVAC_ENOSYS with the message that names the limit
    if (c->prf.enc_plan_limit == kEncPlanLimitDefault)
        return fail(c, PVAC_ENOSYS, std::string(who) + ": noise plan beyond 256 pre-merge edges per half (depth hint > 124 with the default Params)");
    return fail(c, PVAC_ENOSYS, std::string(who) + ": noise plan beyond " + std::to_string(c->prf.enc_plan_limit) +
                                    " pre-merge edges per half (the context's plan limit, pvac_hip_ctx_set_enc_plan_limit)");
}
struct item_plan {
    uint32_t z2, z3, npre, halves;
};
// pvac_hip_enc_items after its argument checks: plans within the limit, capacities checked
int run_enc_items(pvac_hip_ctx* c, size_t n, const pvac_enc_item* items, const std::vector<item_plan>& plans, const uint64_t* rnd,
                  pvac_ct_batch* C, uint32_t flags, uint32_t* status);
}  // namespace

int pvac_hip_enc_caps(pvac_hip_ctx* c, uint32_t* layers_per_value, uint32_t* edges_per_value, uint32_t* draws_hint) {
    return pvac_hip_enc_caps_depth(c, 0, layers_per_value, edges_per_value, draws_hint);
}

int pvac_hip_enc_caps_depth(pvac_hip_ctx* c, int depth_hint, uint32_t* layers_per_value, uint32_t* edges_per_value,
                            uint32_t* draws_hint) try {
    if (!c) return PVAC_EINVAL;
    uint32_t z2, z3;
    plan_noise(c, depth_hint, z2, z3);
    if (plan_over(c, z2, z3)) return plan_refused(c, "enc_caps");
    const uint32_t npre = 8 + 2 * z2 + 3 * z3;
    if (layers_per_value) *layers_per_value = 2;
    if (edges_per_value) *edges_per_value = 2 * npre;
    // mask 2 + per half: nonce 2, signal 2*8 + 2*7, salts npre, noise picks/signs/coefficients, shuffle,
    // and the slack (32 per half up to 256 edges, growing with the plan above: enc_wide.hpp)
    if (draws_hint) *draws_hint = (uint32_t)enc_draws_hint(z2, z3, c->prm.B, 2);
    return PVAC_OK;
} catch (...) { return caught(c, "enc_caps"); }

int pvac_hip_enc_value(pvac_hip_ctx* c, size_t n, const uint64_t* values, const uint64_t* rnd, uint32_t rnd_stride,
                       pvac_ct_batch* C, uint32_t flags, uint32_t* status) {
    return pvac_hip_enc_value_depth(c, n, values, rnd, rnd_stride, 0, C, flags, status);
}

int pvac_hip_enc_value_depth(pvac_hip_ctx* c, size_t n, const uint64_t* values, const uint64_t* rnd, uint32_t rnd_stride,
                             int depth_hint, pvac_ct_batch* C, uint32_t flags, uint32_t* status) try {
    if (!c || !C || (n && (!values || !rnd || !status))) return fail(c, PVAC_EINVAL, "enc_value: arguments");
    if (!C->l_off || !C->l_cnt || !C->layers || !C->e_off || !C->e_cnt || !C->meta || !C->w_lo || !C->w_hi)
        return fail(c, PVAC_EINVAL, "enc_value: output arrays");
    const bool with_sigma = (flags & PVAC_ENC_WITH_SIGMA) != 0;
    if (with_sigma && (!C->sigma || !c->H.ready || C->sigma_words != c->prm.m_bits / 64))
        return fail(c, PVAC_EINVAL, "enc_value: WITH_SIGMA needs C->sigma (m_bits/64 words per edge) and H");
    if (!c->powg.get()) return fail(c, PVAC_EINVAL, "enc_value: powg_B not set (pvac_hip_ctx_set_powg)");
    C->n = n;
    if (!n) return PVAC_OK;
    prf_consts k{};
    int rc = prf_setup(c, k);
    if (rc) return rc;
    enc_plan_args a{};
    a.values = values;
    a.rnd = rnd;
    a.stride = rnd_stride;
    a.B = c->prm.B;
    plan_noise(c, depth_hint, a.Z2, a.Z3);
    a.n = n;
    a.canon = c->prm.canon_tag;
    a.powg = c->powg.get();
    if (plan_over(c, a.Z2, a.Z3)) return plan_refused(c, "enc_value");
    const uint32_t npre = 8 + 2 * a.Z2 + 3 * a.Z3;
    if (npre > kEncPreMax) {   // VALUE items on the wide route: the same layout, value i's draws at rnd + i rnd_stride
        std::vector<uint64_t> v(n);
        hipError_t ev = hipMemcpyAsync(v.data(), values, n * 8, hipMemcpyDeviceToHost, c->stream);
        if (ev == hipSuccess) ev = hipStreamSynchronize(c->stream);
        if (ev != hipSuccess) return hip_fail(c, ev, "enc_value (values)");
        std::vector<pvac_enc_item> items(n);
        for (size_t i = 0; i < n; ++i)
            items[i] = pvac_enc_item{v[i], 0, depth_hint, PVAC_ENC_ITEM_VALUE, (uint64_t)i * rnd_stride, rnd_stride};
        const std::vector<item_plan> plans(n, item_plan{a.Z2, a.Z3, npre, 2});
        return run_enc_items(c, n, items.data(), plans, rnd, C, flags, status);
    }
    const uint64_t cores = (uint64_t)n * enc_cores_per_value(a.Z2, a.Z3);
    const uint64_t pe = (uint64_t)n * 2 * npre;
    const uint32_t sw = c->prm.m_bits / 64;
    // arena: halves | requests | cores | pre CSR (4 x n) | pre layers | meta, w_lo, w_hi, salt | sigma
    auto al = [](uint64_t b) { return (b + 255) & ~255ull; };
    const uint64_t off_req = al((uint64_t)2 * n * enc_half_bytes(npre));
    const uint64_t off_core = off_req + al(cores * prf_request_bytes());
    const uint64_t off_csr = off_core + al(cores * 16);
    const uint64_t off_lay = off_csr + al((uint64_t)n * 32);
    const uint64_t off_e = off_lay + al((uint64_t)n * 2 * sizeof(pvac_layer));
    const uint64_t off_sig = off_e + al(pe * 32);
    const uint64_t total = off_sig + (with_sigma ? al(pe * sw * 8) : 0);
    if (const hipError_t ea = c->prf.enc_arena.grow(total, total)) return hip_fail(c, ea, "alloc enc scratch");
    uint8_t* A = c->prf.enc_arena.get();
    pvac_ct_batch pre{};
    pre.n = n;
    pre.l_off = (uint64_t*)(A + off_csr);
    pre.l_cnt = pre.l_off + n;
    pre.e_off = pre.l_cnt + n;
    pre.e_cnt = pre.e_off + n;
    pre.layers = (pvac_layer*)(A + off_lay);
    pre.meta = (uint64_t*)(A + off_e);
    pre.w_lo = pre.meta + pe;
    pre.w_hi = pre.w_lo + pe;
    uint64_t* pre_salt = pre.w_hi + pe;
    pre.sigma = with_sigma ? (uint64_t*)(A + off_sig) : nullptr;
    pre.sigma_words = with_sigma ? sw : 0;
    scoped_timer t(c, "enc_value");
    hipError_t e = launch_enc_plan(a, A, (prf_request*)(A + off_req), pre, pre_salt, status, c->stream);
    if (e == hipSuccess) e = launch_prf_cores(k, A + off_req, cores, (uint64_t*)(A + off_core), c->stream);
    if (e == hipSuccess) e = launch_enc_weights(a, A, (const uint64_t*)(A + off_core), pre, c->stream);
    if (e == hipSuccess && with_sigma) e = launch_sigma(c->H, c->prm, pre, pre_salt, nullptr, c->num_cus, c->stream);
    pvac_ct_batch out = *C;
    if (!with_sigma) out.sigma = nullptr;
    if (e == hipSuccess) e = launch_enc_finish(a, A, pre, out, status, c->stream);
    if (e == hipSuccess) {   // pvac_hip_enc_path_count: n narrow items, one sub-batch, one run
        c->prf.enc_path[0] += n;
        ++c->prf.enc_path[2];
        ++c->prf.enc_path[3];
    }
    return hip_fail(c, e, "enc_value");
} catch (...) { return caught(c, "enc_value"); }

// ---------------------------------------------------------------- enc_items
namespace {
// kinds and plans of a batch of items; PVAC_EINVAL / PVAC_ENOSYS before anything else happens
int plan_items(pvac_hip_ctx* c, size_t n, const pvac_enc_item* items, std::vector<item_plan>& plans, const char* who) {
    plans.resize(n);
    for (size_t i = 0; i < n; ++i) {
        if (items[i].kind != PVAC_ENC_ITEM_FP && items[i].kind != PVAC_ENC_ITEM_VALUE)
            return fail(c, PVAC_EINVAL, std::string(who) + ": unknown item kind");
        item_plan& p = plans[i];
        plan_noise(c, items[i].depth_hint, p.z2, p.z3);
        if (plan_over(c, p.z2, p.z3)) return plan_refused(c, who);
        p.npre = 8 + 2 * p.z2 + 3 * p.z3;
        p.halves = items[i].kind == PVAC_ENC_ITEM_VALUE ? 2 : 1;
    }
    return PVAC_OK;
}
}  // namespace

int pvac_hip_enc_items_caps(pvac_hip_ctx* c, size_t n, const pvac_enc_item* items, uint64_t* layer_slots,
                            uint64_t* edge_slots, uint64_t* draws_hint) try {
    if (!c || (n && !items)) return fail(c, PVAC_EINVAL, "enc_items_caps: arguments");
    std::vector<item_plan> plans;
    const int rc = plan_items(c, n, items, plans, "enc_items_caps");
    if (rc) return rc;
    uint64_t ls = 0, es = 0;
    for (size_t i = 0; i < n; ++i) {
        const item_plan& p = plans[i];
        ls += p.halves;
        es += (uint64_t)p.halves * p.npre;
        // per half: nonce 2, signal 2*8 + 2*7, salts npre, noise picks/signs/coefficients, shuffle; a value's mask 2;
        // the slack is 32 per half up to 256 edges and grows with the plan above (enc_wide.hpp)
        if (draws_hint) draws_hint[i] = enc_draws_hint(p.z2, p.z3, c->prm.B, p.halves);
    }
    if (layer_slots) *layer_slots = ls;
    if (edge_slots) *edge_slots = es;
    return PVAC_OK;
} catch (...) { return caught(c, "enc_items_caps"); }

int pvac_hip_enc_items(pvac_hip_ctx* c, size_t n, const pvac_enc_item* items, const uint64_t* rnd, uint64_t rnd_words,
                       pvac_ct_batch* C, uint64_t layer_cap, uint64_t edge_cap, uint32_t flags, uint32_t* status) try {
    if (!c || !C || (n && (!items || !rnd || !status))) return fail(c, PVAC_EINVAL, "enc_items: arguments");
    if (!C->l_off || !C->l_cnt || !C->layers || !C->e_off || !C->e_cnt || !C->meta || !C->w_lo || !C->w_hi)
        return fail(c, PVAC_EINVAL, "enc_items: output arrays");
    const bool with_sigma = (flags & PVAC_ENC_WITH_SIGMA) != 0;
    if (with_sigma && (!C->sigma || !c->H.ready || C->sigma_words != c->prm.m_bits / 64))
        return fail(c, PVAC_EINVAL, "enc_items: WITH_SIGMA needs C->sigma (m_bits/64 words per edge) and H");
    if (!c->powg.get()) return fail(c, PVAC_EINVAL, "enc_items: powg_B not set (pvac_hip_ctx_set_powg)");
    if (n > 0x7FFFFFFFull) return fail(c, PVAC_EINVAL, "enc_items: more than 2^31 - 1 items");
    std::vector<item_plan> plans;
    int rc = plan_items(c, n, items, plans, "enc_items");
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i)
        if (items[i].rnd_off > rnd_words || items[i].rnd_cnt > rnd_words - items[i].rnd_off)
            return fail(c, PVAC_EINVAL, "enc_items: an item's draw range lies outside rnd_words");
    uint64_t halves = 0, pe = 0;
    for (size_t i = 0; i < n; ++i) {
        halves += plans[i].halves;
        pe += (uint64_t)plans[i].halves * plans[i].npre;
    }
    if (halves > layer_cap || pe > edge_cap)
        return fail(c, PVAC_ENOMEM, "enc_items: layer_cap / edge_cap below pvac_hip_enc_items_caps");
    C->n = n;
    if (!n) return PVAC_OK;
    return run_enc_items(c, n, items, plans, rnd, C, flags, status);
} catch (...) { return caught(c, "enc_items"); }

}  // extern "C"

namespace {
// A call of narrow items within the budget: one sub-batch, the launches of k_enc_items.hip alone
int run_enc_items_narrow(pvac_hip_ctx* c, size_t n, const pvac_enc_item* items, const std::vector<item_plan>& plans,
                         const uint64_t* rnd, pvac_ct_batch* C, bool with_sigma, uint32_t* status) {
    // one host image: records | work list | permutation (uploaded in one copy)
    std::vector<enc_item_rec> recs(n);
    std::vector<uint64_t> work;
    uint64_t halves = 0, pe = 0, cores = 0;
    for (size_t i = 0; i < n; ++i) {
        const item_plan& p = plans[i];
        enc_item_rec& r = recs[i];
        r.v_lo = items[i].v_lo;
        r.v_hi = items[i].v_hi;
        r.rnd_off = items[i].rnd_off;
        r.rnd_cnt = (uint32_t)std::min<uint64_t>(items[i].rnd_cnt, 0xFFFFFFFFull);
        r.Z2 = p.z2;
        r.Z3 = p.z3;
        r.halves = p.halves;
        r.half_off = halves;
        r.pre_off = pe;
        r.req_off = cores;
        for (uint32_t h = 0; h < p.halves; ++h)
            for (uint32_t g = 0; g <= p.z2 + p.z3; ++g) work.push_back((halves + h) << 16 | g);
        halves += p.halves;
        pe += (uint64_t)p.halves * p.npre;
        cores += (uint64_t)p.halves * 3 * std::max(p.z2 + p.z3, 1u);
    }
    std::vector<uint32_t> perm(n);
    for (size_t i = 0; i < n; ++i) perm[i] = (uint32_t)i;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) {
        return (uint64_t)plans[x].npre * plans[x].halves > (uint64_t)plans[y].npre * plans[y].halves;
    });
    prf_consts k{};
    int rc = prf_setup(c, k);
    if (rc) return rc;
    const uint32_t sw = c->prm.m_bits / 64;
    // arena: records | work | perm | headers | requests | cores | pre CSR (4 x n) | pre layers |
    // meta, w_lo, w_hi, salt, rlo, rhi | key | grp, slot | sigma
    auto al = [](uint64_t b) { return (b + 255) & ~255ull; };
    const uint64_t off_work = al(n * sizeof(enc_item_rec));
    const uint64_t off_perm = off_work + al(work.size() * 8);
    const uint64_t up_bytes = off_perm + al(n * 4);
    const uint64_t off_hdr = up_bytes;
    const uint64_t off_req = off_hdr + al(halves * sizeof(enc_half_hdr));
    const uint64_t off_core = off_req + al(cores * prf_request_bytes());
    const uint64_t off_csr = off_core + al(cores * 16);
    const uint64_t off_lay = off_csr + al((uint64_t)n * 32);
    const uint64_t off_e = off_lay + al(halves * sizeof(pvac_layer));
    const uint64_t off_key = off_e + al(pe * 48);
    const uint64_t off_grp = off_key + al(pe * 4);
    const uint64_t off_sig = off_grp + al(pe * 2);
    const uint64_t total = off_sig + (with_sigma ? al(pe * sw * 8) : 0);
    if (const hipError_t ea = c->prf.enc_arena.grow(total, total)) return hip_fail(c, ea, "alloc enc scratch");
    uint8_t* A = c->prf.enc_arena.get();
    std::vector<uint8_t> img(up_bytes, 0);
    std::memcpy(img.data(), recs.data(), n * sizeof(enc_item_rec));
    std::memcpy(img.data() + off_work, work.data(), work.size() * 8);
    std::memcpy(img.data() + off_perm, perm.data(), n * 4);
    if (const hipError_t eu = upload_words(c, A, img.data(), up_bytes)) return hip_fail(c, eu, "enc_items (upload)");
    pvac_ct_batch pre{};
    pre.n = n;
    pre.l_off = (uint64_t*)(A + off_csr);
    pre.l_cnt = pre.l_off + n;
    pre.e_off = pre.l_cnt + n;
    pre.e_cnt = pre.e_off + n;
    pre.layers = (pvac_layer*)(A + off_lay);
    pre.meta = (uint64_t*)(A + off_e);
    pre.w_lo = pre.meta + pe;
    pre.w_hi = pre.w_lo + pe;
    pre.sigma = with_sigma ? (uint64_t*)(A + off_sig) : nullptr;
    pre.sigma_words = with_sigma ? sw : 0;
    enc_items_args a{};
    a.n = n;
    a.n_work = work.size();
    a.n_halves = halves;
    a.recs = (const enc_item_rec*)A;
    a.work = (const uint64_t*)(A + off_work);
    a.perm = (const uint32_t*)(A + off_perm);
    a.rnd = rnd;
    a.powg = c->powg.get();
    a.canon = c->prm.canon_tag;
    a.B = c->prm.B;
    a.hdr = (enc_half_hdr*)(A + off_hdr);
    a.salt = pre.w_hi + pe;
    a.rlo = a.salt + pe;
    a.rhi = a.rlo + pe;
    a.key = (uint32_t*)(A + off_key);
    a.grp = A + off_grp;
    a.slot = a.grp + pe;
    // timers: the whole sequence, and each launch under its own name (pvac_hip_timing_get)
    scoped_timer t(c, "enc_items");
    auto timed = [&](const char* name, auto&& launch) {
        scoped_timer tk(c, name);
        return launch();
    };
    hipError_t e = timed("enc_items_plan", [&] { return launch_enc_items_plan(a, (prf_request*)(A + off_req), pre, status, c->stream); });
    if (e == hipSuccess)
        e = timed("enc_items_prf", [&] { return launch_prf_cores(k, A + off_req, cores, (uint64_t*)(A + off_core), c->stream); });
    if (e == hipSuccess)
        e = timed("enc_items_weights", [&] { return launch_enc_items_weights(a, (const uint64_t*)(A + off_core), pre, c->stream); });
    if (e == hipSuccess && with_sigma)
        e = timed("enc_items_sigma", [&] { return launch_sigma(c->H, c->prm, pre, a.salt, nullptr, c->num_cus, c->stream); });
    pvac_ct_batch out = *C;
    if (!with_sigma) out.sigma = nullptr;
    if (e == hipSuccess) e = timed("enc_items_finish", [&] { return launch_enc_items_finish(a, pre, out, status, c->stream); });
    return hip_fail(c, e, "enc_items");
}

// One sub-batch [i0, i1) of a call on the mixed path: the narrow items through k_enc_items.hip over a
// compact record list (their index entries and status land in scratch and are scattered to their
// places), the wide items through k_enc_wide.hip. Items, halves and pre-edge slots are numbered from
// the sub-batch's first; base_l / base_e are its first layer and edge slot in C.
int run_enc_sub(pvac_hip_ctx* c, const prf_consts& k, const pvac_enc_item* items, const std::vector<item_plan>& plans, size_t i0,
                size_t i1, uint64_t base_l, uint64_t base_e, const uint64_t* rnd, pvac_ct_batch* C, bool with_sigma, bool wide_all,
                uint32_t* status) {
    const uint32_t B = c->prm.B, sw = c->prm.m_bits / 64;
    std::vector<enc_item_rec> rn, rw;
    std::vector<uint32_t> nid, wid, half_item;
    std::vector<uint64_t> work_n, work_w, fin;
    uint64_t halves = 0, pe = 0, cores = 0;
    for (size_t i = i0; i < i1; ++i) {
        const item_plan& p = plans[i];
        const bool wide = wide_all || p.npre > kEncPreMax;
        enc_item_rec r{};
        r.v_lo = items[i].v_lo;
        r.v_hi = items[i].v_hi;
        r.rnd_off = items[i].rnd_off;
        r.rnd_cnt = (uint32_t)std::min<uint64_t>(items[i].rnd_cnt, 0xFFFFFFFFull);
        r.Z2 = p.z2;
        r.Z3 = p.z3;
        r.halves = p.halves;
        r.half_off = halves;
        r.pre_off = pe;
        r.req_off = cores;
        (wide ? rw : rn).push_back(r);
        (wide ? wid : nid).push_back((uint32_t)(i - i0));
        for (uint32_t h = 0; h < p.halves; ++h) {
            half_item.push_back((uint32_t)(i - i0) << 1 | h);
            for (uint32_t g = 0; g <= p.z2 + p.z3; ++g)
                if (wide) work_w.push_back((halves + h) << 32 | g);
                else work_n.push_back((halves + h) << 16 | g);
            if (wide)   // a half merges down to at most 2 B edges
                for (uint32_t s0 = 0; s0 < std::min<uint64_t>(p.npre, 2ull * B); s0 += kEncWideFinChunk)
                    fin.push_back((halves + h) << 32 | s0);
        }
        halves += p.halves;
        pe += (uint64_t)p.halves * p.npre;
        cores += (uint64_t)p.halves * 3 * std::max(p.z2 + p.z3, 1u);
    }
    const uint64_t nn = rn.size(), nw = rw.size();
    std::vector<uint32_t> perm(nn);   // the narrow plan kernel's order: largest plan first
    for (size_t t = 0; t < nn; ++t) perm[t] = (uint32_t)t;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) {
        return (uint64_t)(8 + 2 * rn[x].Z2 + 3 * rn[x].Z3) * rn[x].halves > (uint64_t)(8 + 2 * rn[y].Z2 + 3 * rn[y].Z3) * rn[y].halves;
    });
    enc_sub_shape sh;
    sh.n = i1 - i0;
    sh.n_narrow = nn;
    sh.n_wide = nw;
    sh.halves = halves;
    sh.pe = pe;
    sh.cores = cores;
    sh.work_narrow = work_n.size();
    sh.work_wide = work_w.size();
    sh.fin = fin.size();
    sh.B = B;
    sh.sigma_words = with_sigma ? sw : 0;
    const enc_sub_layout L = enc_sub_layout_of(sh, sizeof(enc_item_rec), sizeof(enc_half_hdr), prf_request_bytes(), sizeof(pvac_layer));
    if (const hipError_t ea = c->prf.enc_arena.grow(L.total, L.total)) return hip_fail(c, ea, "alloc enc scratch");
    uint8_t* A = c->prf.enc_arena.get();
    std::vector<uint8_t> img(L.up_bytes, 0);
    auto put = [&](uint64_t off, const void* p, size_t bytes) { if (bytes) std::memcpy(img.data() + off, p, bytes); };
    put(L.recs_narrow, rn.data(), nn * sizeof(enc_item_rec));
    put(L.recs_wide, rw.data(), nw * sizeof(enc_item_rec));
    put(L.nid, nid.data(), nn * 4);
    put(L.wid, wid.data(), nw * 4);
    put(L.perm, perm.data(), nn * 4);
    put(L.work_narrow, work_n.data(), work_n.size() * 8);
    put(L.work_wide, work_w.data(), work_w.size() * 8);
    put(L.fin, fin.data(), fin.size() * 8);
    put(L.half_item, half_item.data(), half_item.size() * 4);
    if (const hipError_t eu = upload_words(c, A, img.data(), L.up_bytes)) return hip_fail(c, eu, "enc_items (upload)");
    // the pre-merge batch: the narrow items' index entries first, then the wide items'
    pvac_ct_batch pre{};
    pre.n = sh.n;
    pre.l_off = (uint64_t*)(A + L.pre_idx);
    pre.l_cnt = pre.l_off + sh.n;
    pre.e_off = pre.l_cnt + sh.n;
    pre.e_cnt = pre.e_off + sh.n;
    pre.layers = (pvac_layer*)(A + L.lay);
    pre.meta = (uint64_t*)(A + L.e);
    pre.w_lo = pre.meta + pe;
    pre.w_hi = pre.w_lo + pe;
    pre.sigma = with_sigma ? (uint64_t*)(A + L.sig) : nullptr;
    pre.sigma_words = with_sigma ? sw : 0;
    enc_items_args a{};
    a.n = nn;
    a.n_work = work_n.size();
    a.n_halves = halves;
    a.recs = (const enc_item_rec*)(A + L.recs_narrow);
    a.work = (const uint64_t*)(A + L.work_narrow);
    a.perm = (const uint32_t*)(A + L.perm);
    a.rnd = rnd;
    a.powg = c->powg.get();
    a.canon = c->prm.canon_tag;
    a.B = B;
    a.hdr = (enc_half_hdr*)(A + L.hdr);
    a.salt = pre.w_hi + pe;
    a.rlo = a.salt + pe;
    a.rhi = a.rlo + pe;
    a.key = (uint32_t*)(A + L.key);
    a.grp = A + L.grp;
    a.slot = a.grp + pe;
    enc_wide_args w{};
    w.n = nw;
    w.n_work = work_w.size();
    w.n_fin = fin.size();
    w.recs = (const enc_item_rec*)(A + L.recs_wide);
    w.item = (const uint32_t*)(A + L.wid);
    w.work = (const uint64_t*)(A + L.work_wide);
    w.fin = (const uint64_t*)(A + L.fin);
    w.half_item = (const uint32_t*)(A + L.half_item);
    w.rnd = rnd;
    w.powg = a.powg;
    w.canon = a.canon;
    w.base_l = base_l;
    w.base_e = base_e;
    w.B = B;
    w.pre_base = (uint32_t)nn;
    w.hdr = a.hdr;
    w.key = a.key;
    w.salt = a.salt;
    w.rlo = a.rlo;
    w.rhi = a.rhi;
    w.occ = (uint32_t*)(A + L.occ);
    w.ord = w.occ + pe;
    w.gstart = w.ord + pe;
    w.slot = w.gstart + pe;
    w.tab = (uint32_t*)(A + L.tab);
    w.dlast = (uint64_t*)(A + L.dlast);
    // C as the sub-batch sees it: index arrays and status from its first item, rows from its first slot
    pvac_ct_batch out = *C;
    out.l_off += i0;
    out.l_cnt += i0;
    out.e_off += i0;
    out.e_cnt += i0;
    out.layers += base_l;
    out.meta += base_e;
    out.w_lo += base_e;
    out.w_hi += base_e;
    out.sigma = with_sigma ? C->sigma + base_e * C->sigma_words : nullptr;
    uint32_t* st = status + i0;
    pvac_ct_batch tmp = out;   // the narrow kernels' index entries, compact
    tmp.l_off = (uint64_t*)(A + L.tmp_idx);
    tmp.l_cnt = tmp.l_off + nn;
    tmp.e_off = tmp.l_cnt + nn;
    tmp.e_cnt = tmp.e_off + nn;
    uint32_t* tmp_st = (uint32_t*)(A + L.tmp_status);
    prf_request* req = (prf_request*)(A + L.req);
    uint64_t* core = (uint64_t*)(A + L.core);
    auto timed = [&](const char* name, auto&& launch) {
        scoped_timer tk(c, name);
        return launch();
    };
    hipError_t e = hipSuccess;
    if (nw) e = hipMemsetAsync(w.tab, 0, nw * 2 * 2 * (uint64_t)B * 4, c->stream);
    if (e == hipSuccess && nn) e = timed("enc_items_plan", [&] { return launch_enc_items_plan(a, req, pre, tmp_st, c->stream); });
    if (e == hipSuccess && nw) e = timed("enc_items_plan_wide", [&] { return launch_enc_wide_replay(w, req, pre, out, st, c->stream); });
    if (e == hipSuccess) e = timed("enc_items_prf", [&] { return launch_prf_cores(k, req, cores, core, c->stream); });
    if (e == hipSuccess && nw) e = timed("enc_items_order_wide", [&] { return launch_enc_wide_order(w, c->stream); });
    if (e == hipSuccess && nn) e = timed("enc_items_weights", [&] { return launch_enc_items_weights(a, core, pre, c->stream); });
    if (e == hipSuccess && nw) e = timed("enc_items_weights_wide", [&] { return launch_enc_wide_weights(w, core, pre, c->stream); });
    if (e == hipSuccess && with_sigma)
        e = timed("enc_items_sigma", [&] { return launch_sigma(c->H, c->prm, pre, a.salt, nullptr, c->num_cus, c->stream); });
    if (e == hipSuccess && nn)
        e = timed("enc_items_finish", [&] {
            const hipError_t ef = launch_enc_items_finish(a, pre, tmp, tmp_st, c->stream);
            return ef != hipSuccess ? ef : launch_enc_scatter_index(nn, (const uint32_t*)(A + L.nid), tmp, tmp_st, base_l, base_e, out, st, c->stream);
        });
    if (e == hipSuccess && nw) e = timed("enc_items_finish_wide", [&] { return launch_enc_wide_finish(w, pre, out, st, c->stream); });
    if (e == hipSuccess) {
        c->prf.enc_path[0] += nn;
        c->prf.enc_path[1] += nw;
        ++c->prf.enc_path[2];
    }
    return hip_fail(c, e, "enc_items");
}

int run_enc_items(pvac_hip_ctx* c, size_t n, const pvac_enc_item* items, const std::vector<item_plan>& plans, const uint64_t* rnd,
                  pvac_ct_batch* C, uint32_t flags, uint32_t* status) {
    const bool with_sigma = (flags & PVAC_ENC_WITH_SIGMA) != 0, wide_all = (flags & PVAC_ENC_WIDE_ALL) != 0;
    C->n = n;
    if (!n) return PVAC_OK;
    std::vector<uint64_t> item_pe(n);
    bool any_wide = wide_all;
    for (size_t i = 0; i < n; ++i) {
        item_pe[i] = (uint64_t)plans[i].halves * plans[i].npre;
        any_wide |= plans[i].npre > kEncPreMax;
    }
    std::vector<size_t> cuts;
    enc_cuts(item_pe.data(), n, c->prf.enc_budget, cuts);
    ++c->prf.enc_path[3];
    if (!any_wide && cuts.size() == 2) {
        const int rc = run_enc_items_narrow(c, n, items, plans, rnd, C, with_sigma, status);
        if (!rc) {
            c->prf.enc_path[0] += n;
            ++c->prf.enc_path[2];
        }
        return rc;
    }
    prf_consts k{};
    int rc = prf_setup(c, k);
    if (rc) return rc;
    scoped_timer t(c, "enc_items");
    uint64_t base_l = 0, base_e = 0;
    for (size_t s = 0; s + 1 < cuts.size(); ++s) {
        rc = run_enc_sub(c, k, items, plans, cuts[s], cuts[s + 1], base_l, base_e, rnd, C, with_sigma, wide_all, status);
        if (rc) return rc;
        for (size_t i = cuts[s]; i < cuts[s + 1]; ++i) {
            base_l += plans[i].halves;
            base_e += item_pe[i];
        }
    }
    return PVAC_OK;
}
}  // namespace

extern "C" {

int pvac_hip_base_R(pvac_hip_ctx* c, const pvac_ct_batch* X, uint64_t* R_out) try {
    if (!c || !batch_ok(X) || (X->n && !R_out)) return fail(c, PVAC_EINVAL, "base_R: arguments");
    if (!X->n) return PVAC_OK;
    prf_consts k{};
    int rc = prf_setup(c, k);
    if (rc) return rc;
    // layer slots are addressed through l_off / l_cnt on the device: gather every slot's seed
    std::vector<uint64_t> lo(X->n), lc(X->n);
    hipError_t e = hipMemcpyAsync(lo.data(), X->l_off, X->n * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(lc.data(), X->l_cnt, X->n * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "base_R (offsets)");
    uint64_t slots = 0;
    for (uint64_t i = 0; i < X->n; ++i) slots = std::max(slots, lo[i] + lc[i]);
    if (!slots) return PVAC_OK;
    rc = ensure_prf_scratch(c, 4 * slots);   // 3 cores per slot + the BASE flags behind them
    if (rc) return rc;
    scoped_timer t(c, "base_R");
    return hip_fail(c, launch_base_R(k, *X, slots, c->prf.req.get(), c->prf.core.get(), R_out, c->stream), "base_R");
} catch (...) { return caught(c, "base_R"); }

int pvac_hip_dec_value(pvac_hip_ctx* c, const pvac_ct_batch* X, const uint64_t* R_base, uint64_t* out,
                       uint32_t* status) try {
    if (!c || !batch_ok(X) || !out || !status || (X->n && !R_base)) return fail(c, PVAC_EINVAL, "dec_value: arguments");
    if (!c->powg.get()) return fail(c, PVAC_EINVAL, "dec_value: powg_B not set (pvac_hip_ctx_set_powg)");
    if (!X->n) return PVAC_OK;
    int rc = ensure_scan(c, X->n);   // no plan scratch: a pending plan stays valid
    if (rc) return rc;
    rc = hip_fail(c, c->prf.dec_roff.grow_floor(X->n), "alloc dec offsets");
    if (rc) return rc;
    // dense per-cipher layer offsets (the batch may be capacity-padded)
    hipError_t e = hipMemcpyAsync(c->prf.dec_roff.get(), X->l_cnt, X->n * 8, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = launch_exclusive_scan_u64(c->prf.dec_roff.get(), X->n, c->scan_scratch.get(), &c->ps.totals[0], c->stream);
    unsigned long long total = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&total, &c->ps.totals[0], 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "dec_value (offsets)");
    const size_t need = dec_scratch_bytes(total);
    e = c->prf.dec_scratch.grow(need, need);
    if (e != hipSuccess) return hip_fail(c, e, "alloc dec scratch");
    scoped_timer t(c, "dec_value");
    return hip_fail(c,
                    launch_dec_value(*X, R_base, c->powg.get(), c->prm.B, c->prf.dec_roff.get(), total, c->prf.dec_scratch.get(), out, status,
                                     c->stream),
                    "dec_value");
} catch (...) { return caught(c, "dec_value"); }

}  // extern "C"
