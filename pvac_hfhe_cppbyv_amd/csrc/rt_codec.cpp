// rt_codec.cpp — the device .ct codec: a resident batch to a byte-exact .ct file image in device memory
// and back (kernels: k_ct_image.hip; the format and the host codec it reproduces: ct_codec.cpp).
#include "ct_image.hpp"
#include "ctx.hpp"

using namespace pvhip;

namespace {

// the geometry the kernels are built for: an edge record fits a tile, a sigma row stays countable
const char* geom_limit(const ct_geom& g, uint32_t sigma_words) {
    if (4ull * g.wpe > kCtTileBytes) return "sigma_bits above 130816 (an edge record larger than a 16 KiB tile)";
    if (sigma_words > 4096) return "sigma_words above 4096";
    return nullptr;
}

// sigma rows of `words` used words at `base` with row stride `stride`: can they move 16 bytes at a time
bool sigma_wide(const uint64_t* base, uint32_t words, uint32_t stride) {
    return base && words % 2 == 0 && stride % 2 == 0 && (uintptr_t)base % 16 == 0;
}

}  // namespace

extern "C" {

int pvac_hip_ct_image_plan(pvac_hip_ctx* c, const pvac_ct_batch* X, uint32_t sigma_bits, uint64_t* pos, uint64_t* bytes) try {
    if (!c || !batch_ok(X) || !pos || !bytes) return fail(c, PVAC_EINVAL, "ct_image_plan: bad arguments");
    c->codec.plan_pos = nullptr;
    const ct_geom g = ct_geom_of(X->sigma ? sigma_bits : 0u);
    if (X->sigma && g.nw > X->sigma_words) return fail(c, PVAC_EINVAL, "ct_image_plan: sigma_bits needs more than sigma_words");
    if (const char* m = geom_limit(g, X->sigma ? X->sigma_words : 0u)) return fail(c, PVAC_ENOSYS, std::string("ct_image_plan: ") + m);
    const uint64_t n = X->n;
    if (n >= 0x7FFFFFFFull) return fail(c, PVAC_ENOSYS, "ct_image_plan: 2^31 - 1 ciphers or more");
    if (n && (!X->layers || !X->meta || !X->w_lo || !X->w_hi)) return fail(c, PVAC_EINVAL, "ct_image_plan: null arrays");
    int rc = ensure_scan(c, n);
    if (rc) return rc;
    hipError_t e = c->codec.sz.grow_floor(n + 1);
    if (e == hipSuccess) e = c->codec.toff.grow_floor(n + 1);
    if (e == hipSuccess) e = c->codec.ctl.grow(kCtImageCtlWords, kCtImageCtlWords);
    if (e != hipSuccess) return hip_fail(c, e, "alloc ct_image scratch");
    unsigned long long* ctl = c->codec.ctl.get();
    e = launch_ct_image_plan(*X, g.nbits, c->codec.sz.get(), c->codec.toff.get(), c->scan_scratch.get(), ctl, pos, c->stream);
    unsigned long long got[4] = {};
    if (e == hipSuccess) e = read_back(c, got, ctl, sizeof got);
    if (e != hipSuccess) return hip_fail(c, e, "ct_image_plan");
    *bytes = kCtFileHdr + got[0];
    if (got[2]) return fail(c, PVAC_EINVAL, "ct_image_plan: a layer's rule is 256 or more");
    c->codec.plan_pos = pos;
    c->codec.plan_n = n;
    c->codec.plan_nbits = g.nbits;
    c->codec.plan_bytes = *bytes;
    c->codec.plan_tiles = got[1];
    c->codec.plan_tile_edges = (uint32_t)got[3];
    return PVAC_OK;
} catch (...) { return caught(c, "ct_image_plan"); }

int pvac_hip_ct_image_write(pvac_hip_ctx* c, const pvac_ct_batch* X, uint32_t sigma_bits, const uint64_t* pos, uint8_t* image,
                            uint64_t cap) try {
    if (!c || !batch_ok(X) || !pos || !image) return fail(c, PVAC_EINVAL, "ct_image_write: bad arguments");
    if ((uintptr_t)image % 16) return fail(c, PVAC_EINVAL, "ct_image_write: image is not 16-byte aligned");
    const ct_geom g = ct_geom_of(X->sigma ? sigma_bits : 0u);
    if (X->sigma && g.nw > X->sigma_words) return fail(c, PVAC_EINVAL, "ct_image_write: sigma_bits needs more than sigma_words");
    if (!c->codec.plan_pos || c->codec.plan_pos != pos || c->codec.plan_n != X->n || c->codec.plan_nbits != g.nbits)
        return fail(c, PVAC_EINVAL, "ct_image_write: pos is not this context's latest image plan of X and sigma_bits");
    if (c->codec.plan_bytes > cap) return fail(c, PVAC_ERANGE, "ct_image_write: the image needs more than cap bytes");
    const bool wide = g.nw && sigma_wide(X->sigma, g.nw, X->sigma_words);
    scoped_timer t(c, "ct_image_write");
    const int rc = hip_fail(c,
                            launch_ct_image_write(*X, g.nbits, pos, c->codec.toff.get(), c->codec.plan_tiles, c->codec.plan_tile_edges, wide,
                                                  c->num_cus, image,
                                                  c->stream),
                            "ct_image_write");
    if (!rc) c->codec.path[wide ? 0 : 1]++;
    return rc;
} catch (...) { return caught(c, "ct_image_write"); }

int pvac_hip_ct_image_parse(pvac_hip_ctx* c, const uint8_t* image, uint64_t len, const uint64_t* pos, uint64_t n,
                            uint32_t sigma_bits, pvac_ct_batch* X, uint64_t layer_cap, uint64_t edge_cap, uint32_t* status) try {
    if (!c || !image || !pos || !X) return fail(c, PVAC_EINVAL, "ct_image_parse: bad arguments");
    if ((uintptr_t)image % 16) return fail(c, PVAC_EINVAL, "ct_image_parse: image is not 16-byte aligned");
    if (n && (!X->l_off || !X->l_cnt || !X->e_off || !X->e_cnt)) return fail(c, PVAC_EINVAL, "ct_image_parse: null index arrays");
    if ((layer_cap && !X->layers) || (edge_cap && (!X->meta || !X->w_lo || !X->w_hi)))
        return fail(c, PVAC_EINVAL, "ct_image_parse: null row arrays");
    const ct_geom g = ct_geom_of(sigma_bits);
    if (X->sigma && g.nw > X->sigma_words) return fail(c, PVAC_EINVAL, "ct_image_parse: sigma_bits needs more than sigma_words");
    if (const char* m = geom_limit(g, X->sigma ? X->sigma_words : 0u)) return fail(c, PVAC_ENOSYS, std::string("ct_image_parse: ") + m);
    if (n >= 0x7FFFFFFFull) return fail(c, PVAC_ENOSYS, "ct_image_parse: 2^31 - 1 ciphers or more");
    if (len < kCtFileHdr || n > (len - kCtFileHdr) / kCtCipherHdr) return fail(c, PVAC_EINVAL, "ct_image_parse: len cannot hold n ciphers");
    int rc = ensure_scan(c, n);
    if (rc) return rc;
    hipError_t e = c->codec.words.grow_floor(5 * (n + 1));
    if (e == hipSuccess) e = c->codec.ctl.grow(kCtImageCtlWords, kCtImageCtlWords);
    if (e != hipSuccess) return hip_fail(c, e, "alloc ct_image scratch");
    unsigned long long* ctl = c->codec.ctl.get();
    const bool wide = sigma_wide(X->sigma, g.nw, X->sigma_words);
    unsigned long long got[5] = {};
    {
        scoped_timer t(c, "ct_image_parse");
        e = launch_ct_image_parse(image, len, pos, n, g.nbits, *X, layer_cap, edge_cap, status, c->codec.words.get(),
                                  c->scan_scratch.get(), ctl, wide, c->num_cus, c->stream);
    }
    if (e == hipSuccess) e = read_back(c, got, ctl, sizeof got);
    if (e != hipSuccess) return hip_fail(c, e, "ct_image_parse");
    if (got[3]) return fail(c, PVAC_EINVAL, "ct_image_parse: malformed image (status 1 marks the ciphers)");
    if (got[0] > layer_cap || got[1] > edge_cap) return fail(c, PVAC_ENOMEM, "ct_image_parse: layer_cap or edge_cap is too small");
    X->n = n;
    c->codec.path[wide ? 2 : 3]++;
    if (got[4]) return fail(c, PVAC_EINVAL, "ct_image_parse: an edge's nbits differs from sigma_bits (status 2 marks the ciphers)");
    return PVAC_OK;
} catch (...) { return caught(c, "ct_image_parse"); }

int pvac_hip_ct_image_path_count(pvac_hip_ctx* c, uint64_t out[4]) {
    if (!c || !out) return PVAC_EINVAL;
    for (int k = 0; k < 4; ++k) out[k] = c->codec.path[k];
    return PVAC_OK;
}

}  // extern "C"
