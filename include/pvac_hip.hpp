// pvac_hip.hpp — header-only C++17 adapter: the pvac-hfhe 0.1.0 by-value ciphertext API on top of
// the MI355X C ABI (pvac_hip.h / libpvac_hip.so).
//
// It is templated on the REFERENCE'S OWN types (include/pvac/core/types.hpp:72-139): any Cipher
// with `L` (Layer{rule, seed{ztag, nonce{lo, hi}}, pa, pb}) and `E` (Edge{layer_id, idx, ch,
// w{lo, hi}, s{nbits, w}}) vectors and any PubKey with `prm{B, m_bits, n_bits, h_col_wt,
// x_col_wt, err_wt, edge_budget}`, `canon_tag` and `H` (vector of BitVec columns). Nothing of
// the reference is copied; a maintainer routes the reference's functions here:
//
//   pvac::ct_mul(pk, A, B)  (ops/arithmetic.hpp:47)  -> pvac_hip::ct_mul(pk, A, B)
//   pvac::ct_add(pk, A, B)  (ops/arithmetic.hpp:12)  -> pvac_hip::ct_add(pk, A, B)
//   pvac::ct_sub(pk, A, B)  (ops/arithmetic.hpp:43)  -> pvac_hip::ct_sub(pk, A, B)
//   pvac::ct_scale(pk, A,s) (ops/arithmetic.hpp:33)  -> pvac_hip::ct_scale(pk, A, s)
//   pvac::ct_neg(pk, A)     (ops/arithmetic.hpp:39)  -> pvac_hip::ct_neg(pk, A)
//   pvac::ct_div_const(pk, A, k) (ops/arithmetic.hpp:108) -> pvac_hip::ct_div_const(pk, A, k)
//   pvac::enc_value(pk, sk, v) (ops/encrypt.hpp:289)  -> pvac_hip::enc_value<Cipher>(pk, sk, v)
//   pvac::dec_value(pk, sk, C) (ops/decrypt.hpp:62)  -> pvac_hip::dec_value(pk, sk, C)
//   saveCts / loadCts          (tests/add.cpp:22-155) -> pvac_hip::save_cts_bytes / load_cts_bytes
// plus batched forms (std::vector of pairs in, std::vector out) that keep one launch per batch, and
// ct_sum / ct_lincomb / ct_lincomb_batch: the fold acc = ct_add(pk, acc, [ct_scale] x_k) of any number
// of ciphers as one call (pvac_hip_ct_lincomb_plan / _exec).
// enc/dec also read pk.H_digest, pk.powg_B, pk.prm.lpn_* and the SecKey's prf_k / lpn_s_bits.
//
// Randomness: like the reference (core/random.hpp:40-110), nonces (2 words per new product
// layer, (la, lb) row-major, lo then hi) and salts (1 word per emitted edge, in emit order) come
// from getrandom(2) one 8-byte draw at a time, in the reference's order for a single ct_mul. A
// caller-supplied source (any callable returning uint64_t) replaces it for reproducible runs.
// Errors: C ABI status codes become pvac_hip::Error (the reference has no error codes and lets
// std::bad_alloc escape, arithmetic.hpp:76).
//
// Build: g++/hipcc -std=c++17 -I<repo>/include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
//        ... -L<repo>/pvac_hfhe_cppbyv_amd/lib -lpvac_hip -L/opt/rocm/lib -lamdhip64
#ifndef PVAC_HIP_HPP
#define PVAC_HIP_HPP

#include <hip/hip_runtime_api.h>
#include <sys/random.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <exception>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iomanip>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <thread>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "pvac_hip.h"

namespace pvac_hip {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

using RandomSource = std::function<uint64_t()>;

// In place of a RandomSource in the batched forms (ct_mul_batch, enc_value_batch, ct_mul_chain): nonces,
// salts and draws are filled on the device by the context's CTR_DRBG (pvac_hip_drbg_fill: AES-256,
// seeded from getrandom), no word is drawn, staged or uploaded by the host. The stream is not the
// reference's draw order, so these forms cannot replay a recorded stream; the RandomSource forms can.
struct DeviceRandom {};
inline constexpr DeviceRandom device_random{};

// One 8-byte getrandom per word, as csprng_u64 does (core/random.hpp:106-110).
inline uint64_t os_random_u64() {
    uint64_t v = 0;
    size_t got = 0;
    while (got < sizeof v) {
        const ssize_t r = getrandom(reinterpret_cast<uint8_t*>(&v) + got, sizeof v - got, 0);
        if (r <= 0) throw Error(PVAC_EDEVICE, "getrandom failed");
        got += (size_t)r;
    }
    return v;
}

namespace detail {

inline void hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) throw Error(PVAC_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// RAII device array of T; alloc() keeps the allocation when it already holds count elements, so
// an engine-owned array reused call after call stops paying hipMalloc / hipFree.
template <class T>
struct dev_array {
    T* p = nullptr;
    size_t n = 0, cap = 0;
    dev_array() = default;
    explicit dev_array(size_t count) { alloc(count); }
    dev_array(const dev_array&) = delete;
    dev_array& operator=(const dev_array&) = delete;
    dev_array(dev_array&& o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = o.cap = 0; }
    ~dev_array() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = cap = 0;
    }
    void alloc(size_t count) {
        n = count;
        if (p && count <= cap) return;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = count ? count : 1;
        hip_ok(hipMalloc(&p, cap * sizeof(T)), "hipMalloc");
    }
    void upload(const T* h, size_t count, hipStream_t s) {
        if (count) hip_ok(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s), "H2D");
    }
    void download(T* h, size_t count, hipStream_t s) const {
        if (count) hip_ok(hipMemcpyAsync(h, p, count * sizeof(T), hipMemcpyDeviceToHost, s), "D2H");
    }
};

// Host arrays that are filled right after they are sized (by a copy or a conversion loop): default-
// initialised, so sizing a few GB of output does not first zero it on one thread.
template <class T>
struct default_init : std::allocator<T> {
    template <class U>
    struct rebind { using other = default_init<U>; };
    using std::allocator<T>::allocator;
    default_init() noexcept = default;
    template <class U>
    default_init(const default_init<U>&) noexcept {}
    template <class U>
    void construct(U* p) noexcept(std::is_nothrow_default_constructible<U>::value) { ::new ((void*)p) U; }
    template <class U, class... Args>
    void construct(U* p, Args&&... args) { ::new ((void*)p) U(std::forward<Args>(args)...); }
};
template <class T>
using hvec = std::vector<T, default_init<T>>;

// The same, in page-locked host memory (hipHostMalloc): copies to and from the device run at the
// link's rate instead of through the runtime's pageable staging. Pinning is slow to set up, so only
// engine-owned arrays that are reused call after call use it. When the runtime refuses to pin (a
// locked-memory limit), the array is ordinary pageable memory instead: slower copies, same results.
struct pinned_registry {   // which live allocations are pinned (deallocate frees them the same way)
    std::mutex mu;
    std::set<void*> pinned;
    static pinned_registry& get() {
        static pinned_registry r;
        return r;
    }
};
template <class T>
struct pinned_alloc : default_init<T> {
    using value_type = T;
    template <class U>
    struct rebind { using other = pinned_alloc<U>; };
    pinned_alloc() noexcept = default;
    template <class U>
    pinned_alloc(const pinned_alloc<U>&) noexcept {}
    T* allocate(size_t count) {
        const size_t bytes = (count ? count : 1) * sizeof(T);
        void* q = nullptr;
        if (hipHostMalloc(&q, bytes, hipHostMallocDefault) == hipSuccess && q) {
            pinned_registry& r = pinned_registry::get();
            std::lock_guard<std::mutex> g(r.mu);
            r.pinned.insert(q);
            return static_cast<T*>(q);
        }
        (void)hipGetLastError();   // the refused pin must not surface as a later launch's error
        q = std::malloc(bytes);
        if (!q) throw std::bad_alloc();
        return static_cast<T*>(q);
    }
    void deallocate(T* q, size_t) noexcept {
        bool was_pinned = false;
        {
            pinned_registry& r = pinned_registry::get();
            std::lock_guard<std::mutex> g(r.mu);
            was_pinned = r.pinned.erase((void*)q) != 0;
        }
        if (was_pinned)
            (void)hipHostFree(q);
        else
            std::free(q);
    }
    template <class U>
    bool operator==(const pinned_alloc<U>&) const noexcept { return true; }
    template <class U>
    bool operator!=(const pinned_alloc<U>&) const noexcept { return false; }
};

// What an array of a batch has one element per (sigma: sigma_words per edge).
enum class rows { cipher, layer, edge, sigma };

// Host SoA image of a batch of reference Ciphers + its device copy.
template <bool Pinned>
struct basic_batch {
    template <class T>
    using vec = std::vector<T, typename std::conditional<Pinned, pinned_alloc<T>, default_init<T>>::type>;
    vec<uint64_t> l_off, l_cnt, e_off, e_cnt, meta, w_lo, w_hi, sigma;
    vec<pvac_layer> layers;
    dev_array<uint64_t> d_l_off, d_l_cnt, d_e_off, d_e_cnt, d_meta, d_w_lo, d_w_hi, d_sigma;
    dev_array<pvac_layer> d_layers;
    uint32_t sigma_words = 0;

    // The nine arrays, stated once: f(host array, device array, the pvac_ct_batch field the device
    // array is seen through, what it has one element per), in the order copies are issued. Release,
    // the views, upload and download below all come from this list.
    template <class F>
    void each(F f) {
        f(l_off, d_l_off, &pvac_ct_batch::l_off, rows::cipher);
        f(l_cnt, d_l_cnt, &pvac_ct_batch::l_cnt, rows::cipher);
        f(e_off, d_e_off, &pvac_ct_batch::e_off, rows::cipher);
        f(e_cnt, d_e_cnt, &pvac_ct_batch::e_cnt, rows::cipher);
        f(layers, d_layers, &pvac_ct_batch::layers, rows::layer);
        f(meta, d_meta, &pvac_ct_batch::meta, rows::edge);
        f(w_lo, d_w_lo, &pvac_ct_batch::w_lo, rows::edge);
        f(w_hi, d_w_hi, &pvac_ct_batch::w_hi, rows::edge);
        f(sigma, d_sigma, &pvac_ct_batch::sigma, rows::sigma);
    }

    // frees every host and device array (an engine-owned batch between calls)
    void release() {
        each([](auto& h, auto& d, auto, rows) {
            typename std::decay<decltype(h)>::type().swap(h);
            d.release();
        });
    }

    // n ciphers over the device arrays: the per-cipher arrays always, the others with the rows, sigma
    // only when asked for as well
    pvac_ct_batch view_of(uint64_t n, bool with_rows, bool with_sigma, uint32_t words) {
        pvac_ct_batch b{};
        b.n = n;
        b.sigma_words = words;
        each([&](auto&, auto& d, auto field, rows r) {
            if (r == rows::cipher || (with_rows && (r != rows::sigma || with_sigma))) b.*field = d.p;
        });
        return b;
    }
    pvac_ct_batch view(bool with_sigma) { return view_of(l_cnt.size(), true, with_sigma, sigma_words); }

    // An output batch of n ciphers in the order a plan / exec pair fills it. Before the plan: the
    // per-cipher arrays and the view a plan takes, with nothing else set (words: ct_lincomb's plan
    // reads sigma_words, the others leave 0).
    void alloc_index(size_t n) { d_l_off.alloc(n); d_l_cnt.alloc(n); d_e_off.alloc(n); d_e_cnt.alloc(n); }
    pvac_ct_batch plan_view(uint32_t words = 0) { return view_of(0, false, false, words); }
    // After it: rows of capacity layer / edge slots (the per-cipher arrays, whose offsets the plan
    // wrote, are kept) and the view exec writes.
    void alloc_rows(size_t n, uint64_t lslots, uint64_t eslots, uint32_t words, bool with_sigma) {
        sigma_words = words;
        const uint64_t count[] = {n, lslots, eslots, eslots * words};
        each([&](auto&, auto& d, auto, rows r) {
            if (r != rows::cipher && (r != rows::sigma || with_sigma)) d.alloc(count[(int)r]);
        });
        l_cnt.resize(n);
    }
    pvac_ct_batch out_view(uint64_t n, bool with_sigma) { return view_of(n, true, with_sigma, sigma_words); }

    // host arrays <- the device arrays of v, asynchronously: the per-cipher arrays of its n ciphers
    // (index) or its rows, sigma when v has it
    void fetch(const pvac_ct_batch& v, bool index, uint64_t n, uint64_t lslots, uint64_t eslots, hipStream_t s) {
        sigma_words = v.sigma_words;
        const uint64_t count[] = {n, lslots, eslots, eslots * sigma_words};
        each([&](auto& h, auto&, auto field, rows r) {
            if ((r == rows::cipher) != index || (r == rows::sigma && !v.sigma)) return;
            h.resize(count[(int)r]);
            if (!h.empty()) hip_ok(hipMemcpyAsync(h.data(), v.*field, h.size() * sizeof h[0], hipMemcpyDeviceToHost, s), "D2H");
        });
    }
};
using batch = basic_batch<false>;
using pinned_batch = basic_batch<true>;

// Runs f(begin, end) over [0, n) on up to hardware_concurrency() threads (AoS <-> SoA conversion
// of large batches; each cipher is independent).
template <class F>
void parallel_ranges(size_t n, F f) {
    const size_t hw = std::max<size_t>(1, std::thread::hardware_concurrency());
    const size_t nt = std::min<size_t>(std::min<size_t>(hw, 32), n / 256 + 1);
    if (nt <= 1) { f(size_t(0), n); return; }
    std::vector<std::thread> th;
    const size_t per = (n + nt - 1) / nt;
    for (size_t t = 0; t < nt; ++t) {
        const size_t b = t * per, e = std::min(n, b + per);
        if (b < e) th.emplace_back([=, &f]() { f(b, e); });
    }
    for (auto& x : th) x.join();
}

template <class CipherT, class Batch>
void to_host(const std::vector<const CipherT*>& cs, uint32_t sigma_words, bool with_sigma, Batch& b) {
    const size_t n = cs.size();
    b.sigma_words = sigma_words;
    b.l_off.resize(n); b.l_cnt.resize(n); b.e_off.resize(n); b.e_cnt.resize(n);
    uint64_t lo = 0, eo = 0;
    for (size_t i = 0; i < n; ++i) {
        b.l_off[i] = lo; b.l_cnt[i] = cs[i]->L.size(); lo += cs[i]->L.size();
        b.e_off[i] = eo; b.e_cnt[i] = cs[i]->E.size(); eo += cs[i]->E.size();
    }
    b.layers.resize(lo);
    b.meta.resize(eo); b.w_lo.resize(eo); b.w_hi.resize(eo);
    if (with_sigma) b.sigma.assign(eo * sigma_words, 0);
    parallel_ranges(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            const CipherT* c = cs[i];
            size_t l = b.l_off[i], e = b.e_off[i];
            for (const auto& L : c->L) {
                pvac_layer& y = b.layers[l++];
                y.rule = (uint32_t)L.rule; y.pa = L.pa; y.pb = L.pb; y.pad = 0;
                y.ztag = L.seed.ztag; y.nonce_lo = L.seed.nonce.lo; y.nonce_hi = L.seed.nonce.hi;
            }
            for (const auto& E : c->E) {
                b.meta[e] = (uint64_t)E.layer_id | ((uint64_t)E.idx << 32) | ((uint64_t)E.ch << 48);
                b.w_lo[e] = E.w.lo; b.w_hi[e] = E.w.hi;
                if (with_sigma) {
                    const size_t k = std::min<size_t>(E.s.w.size(), sigma_words);
                    if (k) std::memcpy(&b.sigma[e * sigma_words], E.s.w.data(), k * 8);
                }
                ++e;
            }
        }
    });
}

template <class Batch>
void upload(Batch& b, hipStream_t s, bool with_sigma) {
    b.each([&](auto& h, auto& d, auto, rows r) {
        if (r == rows::sigma && !with_sigma) return;
        d.alloc(h.size());
        d.upload(h.data(), h.size(), s);
    });
}

// host SoA image (c.l_off ... c.sigma filled) -> reference Ciphers
template <class CipherT, class Batch>
std::vector<CipherT> convert_host(Batch& c, size_t n, uint32_t m_bits, bool with_sigma) {
    std::vector<CipherT> out(n);
    parallel_ranges(n, [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; ++i) {
        CipherT& C = out[i];
        C.L.resize(c.l_cnt[i]);
        for (size_t l = 0; l < c.l_cnt[i]; ++l) {
            const pvac_layer& y = c.layers[c.l_off[i] + l];
            auto& L = C.L[l];
            L.rule = static_cast<decltype(L.rule)>(y.rule);
            L.pa = y.pa; L.pb = y.pb;
            L.seed.ztag = y.ztag; L.seed.nonce.lo = y.nonce_lo; L.seed.nonce.hi = y.nonce_hi;
        }
        C.E.resize(c.e_cnt[i]);
        for (size_t k = 0; k < c.e_cnt[i]; ++k) {
            const size_t e = c.e_off[i] + k;
            auto& E = C.E[k];
            E.layer_id = (uint32_t)c.meta[e];
            E.idx = (uint16_t)(c.meta[e] >> 32);
            E.ch = (uint8_t)(c.meta[e] >> 48);
            E.w.lo = c.w_lo[e]; E.w.hi = c.w_hi[e];
            // weights-only results (an engine extension: the reference always draws sigma) keep an
            // empty BitVec instead of a zeroed m_bits one (1 KiB per edge); save_cts zero-pads it
            if (with_sigma) {
                E.s.nbits = m_bits;
                E.s.w.assign(&c.sigma[e * c.sigma_words], &c.sigma[e * c.sigma_words] + c.sigma_words);
            }
        }
    }
    });
    return out;
}

// device records of the view v (n ciphers; lslots / eslots rows) -> host SoA image c, synchronous
template <class Batch>
void download(Batch& c, const pvac_ct_batch& v, size_t n, uint64_t lslots, uint64_t eslots, hipStream_t s) {
    c.fetch(v, true, n, lslots, eslots, s);
    c.fetch(v, false, n, lslots, eslots, s);
    hip_ok(hipStreamSynchronize(s), "sync");
}

template <class CipherT>
std::vector<CipherT> from_device(batch& c, size_t n, uint64_t lslots, uint64_t eslots, uint32_t m_bits,
                                 bool with_sigma, hipStream_t s) {
    download(c, c.out_view(n, with_sigma), n, lslots, eslots, s);
    return convert_host<CipherT>(c, n, m_bits, with_sigma);
}

// a small device array -> host, synchronous (a status or digest array; an array of a batch view
// handed to a chain hook, valid only there)
template <class T>
hvec<T> d2h(const T* p, size_t n, hipStream_t s) {
    hvec<T> v(n);
    if (n) hip_ok(hipMemcpyAsync(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost, s), "D2H");
    hip_ok(hipStreamSynchronize(s), "sync");
    return v;
}

// the used rows of a capacity-padded device batch view -> reference Ciphers: the per-cipher arrays
// first, which say how many rows there are
template <class CipherT>
std::vector<CipherT> from_view(const pvac_ct_batch& v, uint32_t m_bits, hipStream_t s) {
    batch c;
    const size_t n = v.n;
    c.fetch(v, true, n, 0, 0, s);
    hip_ok(hipStreamSynchronize(s), "sync");
    uint64_t nl = 0, ne = 0;
    for (size_t i = 0; i < n; ++i) {
        nl = std::max(nl, c.l_off[i] + c.l_cnt[i]);
        ne = std::max(ne, c.e_off[i] + c.e_cnt[i]);
    }
    c.fetch(v, false, n, nl, ne, s);
    hip_ok(hipStreamSynchronize(s), "sync");
    return convert_host<CipherT>(c, n, m_bits, v.sigma != nullptr);
}

// The ragged term lists of a ct_lincomb call as the C ABI takes them (pvac_lincomb, host side):
// seg_off has one entry more than there are outputs, scale 2 words (lo, hi) per term or none, flags
// one word per term or none (none with scales: every term is scaled).
struct lincomb_lists {
    std::vector<uint64_t> seg_off, term, scale;
    std::vector<uint32_t> flags;
};

// Checks a call against a pool of n_x ciphers and flattens the scales: seg_off starts at 0, does not
// decrease and ends at term.size() (an empty seg_off is no output at all); every term is below n_x;
// scales and flags are empty or one per term, flags only with scales. Pure host arithmetic
// (tests/cpp/lincomb_flatten_check.cpp).
template <class FpT>
lincomb_lists flatten_lincomb(size_t n_x, const std::vector<uint64_t>& seg_off, const std::vector<uint64_t>& term,
                              const std::vector<FpT>& scales, const std::vector<uint32_t>& flags) {
    lincomb_lists s;
    s.seg_off = seg_off;
    if (s.seg_off.empty()) s.seg_off.push_back(0);
    if (s.seg_off.front() != 0 || s.seg_off.back() != term.size())
        throw Error(PVAC_EINVAL, "ct_lincomb: seg_off must run from 0 to the number of terms");
    for (size_t i = 1; i < s.seg_off.size(); ++i)
        if (s.seg_off[i] < s.seg_off[i - 1]) throw Error(PVAC_EINVAL, "ct_lincomb: seg_off decreases");
    for (const uint64_t t : term)
        if (t >= n_x) throw Error(PVAC_EINVAL, "ct_lincomb: a term index beyond the pool");
    if ((!scales.empty() && scales.size() != term.size()) || (!flags.empty() && flags.size() != term.size()) ||
        (scales.empty() && !flags.empty()))
        throw Error(PVAC_EINVAL, "ct_lincomb: scales / flags are one per term (flags only with scales)");
    s.term = term;
    s.scale.reserve(2 * scales.size());
    for (const FpT& f : scales) {
        s.scale.push_back(f.lo);
        s.scale.push_back(f.hi);
    }
    s.flags = flags;
    return s;
}

}  // namespace detail

// One device context per (device, canon_tag); owns the device copy of pk.H for sigma.
// A batch resident on the device that owns its arrays (Engine::batch_from_image).
struct device_batch {
    detail::batch arrays;
    uint32_t sigma_bits = 0;   // nbits of every edge's sigma in the file it came from (0: no sigma rows)
    pvac_ct_batch view() { return arrays.view(sigma_bits != 0); }
};

class Engine {
public:
    Engine(int device, const pvac_hip_params& prm) : prm_(prm) {
        const int rc = pvac_hip_ctx_create(device, &prm, &ctx_);
        if (rc) throw Error(rc, "pvac_hip_ctx_create failed (no MI355X / HIP runtime?)");
        stream_ = (hipStream_t)pvac_hip_ctx_stream(ctx_);
    }
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;
    ~Engine() {
        if (stream_) (void)hipStreamSynchronize(stream_);
        release_mul();
        pvac_hip_ctx_destroy(ctx_);
    }

    template <class PubKeyT>
    static pvac_hip_params params_of(const PubKeyT& pk) {
        pvac_hip_params p{};
        p.B = (uint32_t)pk.prm.B; p.m_bits = (uint32_t)pk.prm.m_bits; p.n_bits = (uint32_t)pk.prm.n_bits;
        p.h_col_wt = (uint32_t)pk.prm.h_col_wt; p.x_col_wt = (uint32_t)pk.prm.x_col_wt;
        p.err_wt = (uint32_t)pk.prm.err_wt; p.edge_budget = (uint64_t)pk.prm.edge_budget;
        p.canon_tag = pk.canon_tag;
        return p;
    }

    pvac_hip_ctx* ctx() const { return ctx_; }
    uint32_t sigma_words() const { return (prm_.m_bits + 63) / 64; }

    // The layers a ct_mul pair may have before compaction, and (with 30000) a ct_add pair in all; ct_lincomb,
    // compact and ct_recrypt below take a term, cipher or sum of max(30000, limit) layers as well
    // (pvac_hip_ctx_set_layer_limit: PVAC_LAYER_LIMIT_DEFAULT .. PVAC_LAYER_LIMIT_MAX; a deep pair's
    // scratch is about 16 words per key slot). The thread-local engines of the free functions keep
    // the default: engine_for(pk).set_layer_limit(n) raises it for the calling thread.
    void set_layer_limit(uint32_t max_layers) { check(pvac_hip_ctx_set_layer_limit(ctx_, max_layers)); }
    uint32_t layer_limit() const {
        uint32_t v = 0;
        if (const int rc = pvac_hip_ctx_layer_limit(ctx_, &v)) throw Error(rc, "pvac_hip_ctx_layer_limit");
        return v;
    }
    // pvac_hip_deep_route_count: ct_lincomb terms on the deep-term route, its fold sums run by the deep add
    // kernel, ciphers above 30000 layers compacted, ct_recrypt sums above 30000 layers, since the engine was made
    std::array<uint64_t, 4> deep_route_counts() const {
        std::array<uint64_t, 4> v{};
        if (const int rc = pvac_hip_deep_route_count(ctx_, v.data())) throw Error(rc, "pvac_hip_deep_route_count");
        return v;
    }

    // The pre-merge edges per half an encryption may plan (pvac_hip_ctx_set_enc_plan_limit:
    // PVAC_ENC_PLAN_LIMIT_DEFAULT = 256 .. PVAC_ENC_PLAN_LIMIT_MAX). Above 256 an item runs the wide route;
    // scratch is about 1 KB per pre-merge edge with sigma and a text's edges grow with the square of its
    // length. The free functions' engine: engine_for(pk).set_enc_plan_limit(n). set_enc_budget: the
    // pre-merge edges of a sub-batch (PVAC_ENC_BUDGET_DEFAULT).
    void set_enc_plan_limit(uint32_t max_pre_edges) { check(pvac_hip_ctx_set_enc_plan_limit(ctx_, max_pre_edges)); }
    uint32_t enc_plan_limit() const {
        uint32_t v = 0;
        if (const int rc = pvac_hip_ctx_enc_plan_limit(ctx_, &v)) throw Error(rc, "pvac_hip_ctx_enc_plan_limit");
        return v;
    }
    void set_enc_budget(uint64_t pre_edges) { check(pvac_hip_ctx_set_enc_budget(ctx_, pre_edges)); }

    // Wall-clock split of the last batched ct_mul, in seconds: host AoS -> SoA, H2D, plan + nonce
    // draws, exec (+ salts, sigma and the device-side pack of the used rows), D2H, SoA -> AoS.
    struct Phases { double to_soa = 0, h2d = 0, plan = 0, exec = 0, d2h = 0, to_aos = 0; };
    const Phases& last_phases() const { return phases_; }

    // Batched ct_mul keeps its host (pinned) and device arrays between calls, sized by the largest
    // batch so far; trim() hands them back.
    void trim() {
        detail::hip_ok(hipStreamSynchronize(stream_), "sync");
        release_mul();
    }

    // H regenerated on the device from canon_tag (gen_H, crypto/matrix.hpp:191-251); returns the
    // H_digest for comparison with pk.H_digest.
    std::vector<uint8_t> gen_H() {
        std::vector<uint8_t> d(32);
        check(pvac_hip_ctx_gen_H(ctx_, d.data()));
        h_ready_ = true;
        return d;
    }

    // pk.H (dense BitVec columns) -> device sparse columns, once; an empty pk.H (e.g. a key
    // loaded without H) is regenerated on the device from canon_tag.
    template <class PubKeyT>
    void ensure_H(const PubKeyT& pk) {
        if (h_ready_) return;
        if (pk.H.empty()) {
            (void)gen_H();
            return;
        }
        const uint32_t wpc = sigma_words();
        std::vector<uint64_t> dense((size_t)pk.H.size() * wpc, 0);
        for (size_t c = 0; c < pk.H.size(); ++c)
            std::memcpy(&dense[c * wpc], pk.H[c].w.data(), std::min<size_t>(pk.H[c].w.size(), wpc) * 8);
        check(pvac_hip_ctx_set_H(ctx_, dense.data(), (uint32_t)pk.H.size(), wpc));
        h_ready_ = true;
    }

    // Batched ct_mul (ops/arithmetic.hpp:47-106) over pairs (A[i], B[i]). with_sigma needs pk.H.
    template <class PubKeyT, class CipherT>
    std::vector<CipherT> ct_mul(const PubKeyT& pk, const std::vector<const CipherT*>& A,
                                const std::vector<const CipherT*>& B, bool with_sigma, const RandomSource& rnd) {
        return ct_mul_from(pk, A, B, with_sigma, &rnd);
    }
    // ... with every nonce and salt from the device generator: nothing is drawn or uploaded by the host
    template <class PubKeyT, class CipherT>
    std::vector<CipherT> ct_mul(const PubKeyT& pk, const std::vector<const CipherT*>& A,
                                const std::vector<const CipherT*>& B, bool with_sigma, DeviceRandom) {
        return ct_mul_from(pk, A, B, with_sigma, nullptr);
    }

private:
    // rnd == nullptr: device_random
    template <class PubKeyT, class CipherT>
    std::vector<CipherT> ct_mul_from(const PubKeyT& pk, const std::vector<const CipherT*>& A,
                                     const std::vector<const CipherT*>& B, bool with_sigma, const RandomSource* rnd) {
        if (A.size() != B.size()) throw Error(PVAC_EINVAL, "ct_mul: |A| != |B|");
        const size_t n = A.size();
        if (!n) return {};
        if (with_sigma) ensure_H(pk);
        using clk = std::chrono::steady_clock;
        auto t = clk::now();
        auto lap = [&t](double& into) {
            const auto u = clk::now();
            into = std::chrono::duration<double>(u - t).count();
            t = u;
        };
        // engine-owned (pinned, grow-only) arrays: a steady stream of batches maps, pins and frees nothing
        detail::pinned_batch& a = mul_a_;
        detail::pinned_batch& b = mul_b_;
        detail::pinned_batch& c = mul_c_;
        detail::to_host(A, sigma_words(), false, a);
        detail::to_host(B, sigma_words(), false, b);
        lap(phases_.to_soa);
        detail::upload(a, stream_, false);
        detail::upload(b, stream_, false);
        detail::hip_ok(hipStreamSynchronize(stream_), "sync");
        lap(phases_.h2d);
        pvac_ct_batch va = a.view(false), vb = b.view(false);
        c.alloc_index(n);
        pvac_ct_batch vc = c.plan_view();
        pvac_hip_plan plan{};
        check(pvac_hip_ct_mul_plan(ctx_, &va, &vb, &vc, &plan));
        detail::dev_array<uint64_t>& d_nonces = mul_nonces_;
        const size_t nonce_words = 2 * (plan.total_layer_slots ? plan.total_layer_slots : 1);
        d_nonces.alloc(nonce_words);
        if (rnd) {
            // nonces per pair in the reference's draw order: (la, lb) row-major, lo then hi
            std::vector<uint64_t> loff(n);
            c.d_l_off.download(loff.data(), n, stream_);
            detail::hip_ok(hipStreamSynchronize(stream_), "sync");
            std::vector<uint64_t> nonces(nonce_words, 0);
            for (size_t i = 0; i < n; ++i) {
                const uint64_t LA = A[i]->L.size(), LB = B[i]->L.size();
                const uint64_t s0 = loff[i] + LA + LB;
                for (uint64_t k = 0; k < LA * LB; ++k) {
                    nonces[2 * (s0 + k)] = (*rnd)();
                    nonces[2 * (s0 + k) + 1] = (*rnd)();
                }
            }
            d_nonces.upload(nonces.data(), nonces.size(), stream_);
        } else {
            // one fill over every layer slot's two words: only the product layers' are read
            check(pvac_hip_drbg_fill(ctx_, d_nonces.p, nonce_words));
        }
        c.alloc_rows(n, plan.total_layer_slots, plan.total_edge_slots, sigma_words(), with_sigma);
        lap(phases_.plan);
        vc = c.out_view(n, false);
        check(pvac_hip_ct_mul_exec(ctx_, &plan, &va, &vb, d_nonces.p, nullptr, &vc, 0));
        if (with_sigma) {
            // one salt per emitted edge, drawn after the weights are known (arithmetic.hpp:90-94), in
            // emit order. In the reference hash order (pair status 0) output position k of a pair IS
            // its k-th emit, so sigma_from_H runs over the finished batch (pvac_hip_sigma_batch);
            // a pair in the canonical order (guard_budget) takes its salts in hash order, which the
            // second exec with PVAC_MUL_WITH_SIGMA maps (salt positions)
            std::vector<uint64_t> ecnt(n), eoff(n);
            std::vector<uint32_t> status(n);
            detail::dev_array<uint32_t>& d_status = mul_status_;
            d_status.alloc(n);
            check(pvac_hip_ct_mul_status(ctx_, d_status.p, n));
            if (rnd) {
                c.d_e_cnt.download(ecnt.data(), n, stream_);
                c.d_e_off.download(eoff.data(), n, stream_);
            }
            d_status.download(status.data(), n, stream_);
            detail::hip_ok(hipStreamSynchronize(stream_), "sync");
            const size_t salt_words = plan.total_edge_slots ? plan.total_edge_slots : 1;
            detail::dev_array<uint64_t>& d_salts = mul_salts_;
            d_salts.alloc(salt_words);
            bool hash_order = true;
            for (size_t i = 0; i < n; ++i) hash_order &= status[i] != 1u;
            if (rnd) {
                std::vector<uint64_t> salts(salt_words, 0);
                for (size_t i = 0; i < n; ++i)
                    for (uint64_t k = 0; k < ecnt[i]; ++k) salts[eoff[i] + k] = (*rnd)();
                d_salts.upload(salts.data(), salts.size(), stream_);
            } else {
                check(pvac_hip_drbg_fill(ctx_, d_salts.p, salt_words));   // a salt per edge slot
            }
            vc = c.out_view(n, true);
            if (hash_order) {
                check(pvac_hip_sigma_batch(ctx_, &vc, d_salts.p));
            } else {
                check(pvac_hip_ct_mul_plan(ctx_, &va, &vb, &vc, &plan));
                vc = c.out_view(n, true);
                check(pvac_hip_ct_mul_exec(ctx_, &plan, &va, &vb, d_nonces.p, d_salts.p, &vc, PVAC_MUL_WITH_SIGMA));
            }
        }
        // only the used rows cross the link: packed on the device first (each pair's output kept its
        // plan capacity), then copied at their exact totals
        detail::pinned_batch& p = mul_p_;
        p.alloc_index(n);
        p.alloc_rows(n, plan.total_layer_slots, plan.total_edge_slots, sigma_words(), with_sigma);
        vc = c.out_view(n, with_sigma);
        pvac_ct_batch vp = p.out_view(n, with_sigma);
        uint64_t tot[2] = {0, 0};
        check(pvac_hip_batch_pack(ctx_, &vc, &vp, tot));
        lap(phases_.exec);
        detail::download(c, vp, n, tot[0], tot[1], stream_);
        lap(phases_.d2h);
        std::vector<CipherT> out = detail::convert_host<CipherT>(c, n, prm_.m_bits, with_sigma);
        lap(phases_.to_aos);
        return out;
    }

public:

    // Depth chains through pvac_hip_ct_mul_chain (the chain entry point): for every input x of xs,
    // c_0 = x, c_k = ct_mul(pk, c_{k-1}, x) for k = 1..depth (the test_depth / cfg-4 shape of
    // tests/test_main.cpp:289-293's loop); returns every c_depth. Randomness of chain i comes from
    // rnds[i] in the reference's draw order, step after step: 2 words per new product layer (la, lb
    // row-major, lo then hi), then one salt per emitted edge (arithmetic.hpp:64, 93). Only c_depth's
    // sigmas survive a chain, so the intermediate salts are drawn and discarded; with_sigma computes
    // the final step's sigmas (needs pk.H), otherwise the final salts are discarded too. A chain
    // replayed from a reference stream is byte-identical to the reference's c_depth. devices: GPU
    // ordinals to spread the chains over (whole chunks per device; empty = this engine's device);
    // chunk: inputs per worker chunk (with sigma the last step holds 1 KiB per edge: keep it small).
    // ops (optional): per-step operands, ops[d][i] the cipher chain i multiplies by at step d + 1
    // (the reference's own loop, tests/test_main.cpp:291-292, multiplies by a fresh enc_value(2) per
    // step); steps past ops.size() multiply by x. rnds then carry only the ct_mul draws: a caller
    // replaying one interleaved stream encrypts the operands from their own stretches of it.
    template <class PubKeyT, class CipherT>
    std::vector<CipherT> ct_mul_chain(const PubKeyT& pk, const std::vector<const CipherT*>& xs, uint32_t depth,
                                      bool with_sigma, std::vector<RandomSource>& rnds,
                                      const std::vector<int>& devices = {}, uint32_t streams = 2, uint64_t chunk = 16,
                                      const std::vector<std::vector<const CipherT*>>& ops = {}) {
        if (rnds.size() != xs.size()) throw Error(PVAC_EINVAL, "ct_mul_chain: one RandomSource per input");
        return chain_from(pk, xs, depth, with_sigma, &rnds, devices, streams, chunk, ops);
    }
    // ... with the workers' device generators (PVAC_CHAIN_DRBG): no hook draws, stages or uploads a word
    template <class PubKeyT, class CipherT>
    std::vector<CipherT> ct_mul_chain(const PubKeyT& pk, const std::vector<const CipherT*>& xs, uint32_t depth,
                                      bool with_sigma, DeviceRandom, const std::vector<int>& devices = {},
                                      uint32_t streams = 2, uint64_t chunk = 16,
                                      const std::vector<std::vector<const CipherT*>>& ops = {}) {
        return chain_from<PubKeyT, CipherT>(pk, xs, depth, with_sigma, nullptr, devices, streams, chunk, ops);
    }

private:
    // rnds == nullptr: device_random
    template <class PubKeyT, class CipherT>
    std::vector<CipherT> chain_from(const PubKeyT& pk, const std::vector<const CipherT*>& xs, uint32_t depth,
                                    bool with_sigma, std::vector<RandomSource>* rnds, const std::vector<int>& devices,
                                    uint32_t streams, uint64_t chunk, const std::vector<std::vector<const CipherT*>>& ops) {
        const size_t n = xs.size();
        if (ops.size() > depth) throw Error(PVAC_EINVAL, "ct_mul_chain: more operand steps than depth");
        for (const auto& y : ops)
            if (y.size() != n) throw Error(PVAC_EINVAL, "ct_mul_chain: one operand per input and step");
        if (!n) return {};
        if (with_sigma) ensure_H(pk);
        detail::batch x;
        pvac_ct_batch vx = stage(xs, false, x);
        std::vector<detail::batch> yb(ops.size());
        std::vector<pvac_ct_batch> yv(ops.size());
        for (size_t d = 0; d < ops.size(); ++d) yv[d] = stage(ops[d], false, yb[d]);
        detail::hip_ok(hipStreamSynchronize(stream_), "sync");
        struct state {
            std::vector<RandomSource>* rnds;
            std::vector<CipherT> out;
            uint32_t depth, m_bits;
            bool sigma;
        } stt{rnds, std::vector<CipherT>(n), depth, prm_.m_bits, with_sigma};
        pvac_chain_opts o{};
        o.depth = depth;
        o.streams = streams;
        o.chunk = chunk;
        o.flags = (with_sigma ? PVAC_MUL_WITH_SIGMA : 0u) | (rnds ? 0u : PVAC_CHAIN_DRBG);
        o.user = &stt;
        o.devices = devices.empty() ? nullptr : devices.data();
        o.n_devices = (uint32_t)devices.size();
        o.operands = yv.empty() ? nullptr : yv.data();
        o.n_operands = (uint32_t)yv.size();
        // hooks run on the library's worker threads; chunks (and so their inputs' sources) are disjoint
        o.nonces_at = [](void* u, uint32_t, uint64_t c0, const pvac_ct_batch* A, const pvac_ct_batch* X,
                         const pvac_ct_batch* C, uint64_t* words, uint64_t nw, void* st) -> int {
            try {
                state& S = *(state*)u;
                const hipStream_t s = (hipStream_t)st;
                const auto la = detail::d2h(A->l_cnt, A->n, s), lx = detail::d2h(X->l_cnt, X->n, s);
                const auto lo = detail::d2h(C->l_off, C->n, s);
                std::vector<uint64_t> w(nw, 0);
                for (size_t i = 0; i < A->n; ++i) {
                    RandomSource& r = (*S.rnds)[c0 + i];
                    const uint64_t s0 = lo[i] + la[i] + lx[i];
                    for (uint64_t k = 0; k < la[i] * lx[i]; ++k) {
                        w[2 * (s0 + k)] = r();
                        w[2 * (s0 + k) + 1] = r();
                    }
                }
                detail::hip_ok(hipMemcpyAsync(words, w.data(), nw * 8, hipMemcpyHostToDevice, s), "H2D");
                detail::hip_ok(hipStreamSynchronize(s), "sync");
                return 0;
            } catch (...) {
                return 1;
            }
        };
        o.after_step = [](void* u, uint32_t step, uint64_t c0, const pvac_ct_batch*, const pvac_ct_batch*,
                          const pvac_ct_batch* C, uint64_t*, uint64_t, void* st) -> int {
            try {
                state& S = *(state*)u;
                if (S.sigma && step + 1 == S.depth) return 0;   // salts_at draws these
                const auto ec = detail::d2h(C->e_cnt, C->n, (hipStream_t)st);
                for (size_t i = 0; i < C->n; ++i)
                    for (uint64_t k = 0; k < ec[i]; ++k) (void)(*S.rnds)[c0 + i]();
                return 0;
            } catch (...) {
                return 1;
            }
        };
        o.salts_at = [](void* u, uint32_t, uint64_t c0, const pvac_ct_batch*, const pvac_ct_batch*,
                        const pvac_ct_batch* C, uint64_t* words, uint64_t nw, void* st) -> int {
            try {
                state& S = *(state*)u;
                const hipStream_t s = (hipStream_t)st;
                const auto ec = detail::d2h(C->e_cnt, C->n, s), eo = detail::d2h(C->e_off, C->n, s);
                std::vector<uint64_t> w(nw ? nw : 1, 0);
                for (size_t i = 0; i < C->n; ++i)
                    for (uint64_t k = 0; k < ec[i]; ++k) w[eo[i] + k] = (*S.rnds)[c0 + i]();
                detail::hip_ok(hipMemcpyAsync(words, w.data(), nw * 8, hipMemcpyHostToDevice, s), "H2D");
                detail::hip_ok(hipStreamSynchronize(s), "sync");
                return 0;
            } catch (...) {
                return 1;
            }
        };
        o.on_chunk = [](void* u, uint64_t c0, const pvac_ct_batch* C, void* st) -> int {
            try {
                state& S = *(state*)u;
                auto cs = detail::from_view<CipherT>(*C, S.m_bits, (hipStream_t)st);
                for (size_t i = 0; i < cs.size(); ++i) S.out[c0 + i] = std::move(cs[i]);
                return 0;
            } catch (...) {
                return 1;
            }
        };
        if (!rnds) o.nonces_at = o.after_step = o.salts_at = nullptr;   // the workers' generators fill
        pvac_chain_stats st{};
        check(pvac_hip_ct_mul_chain(ctx_, &vx, &o, &st));
        return std::move(stt.out);
    }

public:

    // Batched ct_add / ct_sub (ops/arithmetic.hpp:12-31, 43-45); sigmas carried through.
    template <class CipherT>
    std::vector<CipherT> ct_add(const std::vector<const CipherT*>& A, const std::vector<const CipherT*>& B, bool negate_b) {
        if (A.size() != B.size()) throw Error(PVAC_EINVAL, "ct_add: |A| != |B|");
        const size_t n = A.size();
        if (!n) return {};
        detail::batch a, b, c;
        pvac_ct_batch va = stage(A, true, a), vb = stage(B, true, b);
        pvac_ct_batch vc = plan_out(c, n);
        pvac_hip_plan plan{};
        check(pvac_hip_ct_add_plan(ctx_, &va, &vb, &vc, &plan));
        vc = exec_out(c, n, plan.total_layer_slots, plan.total_edge_slots, sigma_words(), true);
        check(pvac_hip_ct_add_exec(ctx_, &plan, &va, &vb, negate_b ? 1 : 0, &vc));
        return detail::from_device<CipherT>(c, n, plan.total_layer_slots, plan.total_edge_slots, prm_.m_bits, true,
                                            stream_);
    }

    // ct_lincomb (pvac_hip_ct_lincomb_plan / _exec): output i is the reference's fold over the terms
    // S.term[S.seg_off[i] .. S.seg_off[i + 1]) of the pool X. with_sigma = false computes weights only
    // (results keep empty BitVecs, as ct_mul's weights-only results do).
    template <class CipherT>
    std::vector<CipherT> ct_lincomb(const std::vector<const CipherT*>& X, const detail::lincomb_lists& S, bool with_sigma) {
        const size_t n = S.seg_off.size() - 1;
        if (!n) return {};
        detail::batch x, c;
        const pvac_ct_batch vx = stage(X, with_sigma, x);
        detail::dev_array<uint64_t> d_so(S.seg_off.size()), d_tm(S.term.size()), d_sc(S.scale.size());
        detail::dev_array<uint32_t> d_fl(S.flags.size());
        d_so.upload(S.seg_off.data(), S.seg_off.size(), stream_);
        d_tm.upload(S.term.data(), S.term.size(), stream_);
        d_sc.upload(S.scale.data(), S.scale.size(), stream_);
        d_fl.upload(S.flags.data(), S.flags.size(), stream_);
        pvac_lincomb s{};
        s.n = n;
        s.n_terms = S.term.size();
        s.seg_off = d_so.p;
        s.term = d_tm.p;
        s.scale = S.scale.empty() ? nullptr : d_sc.p;
        s.flags = S.flags.empty() ? nullptr : d_fl.p;
        pvac_ct_batch vc = plan_out(c, n, sigma_words());
        pvac_hip_plan plan{};
        check(pvac_hip_ct_lincomb_plan(ctx_, &vx, &s, &vc, &plan));
        vc = exec_out(c, n, plan.total_layer_slots, plan.total_edge_slots, sigma_words(), with_sigma);
        check(pvac_hip_ct_lincomb_exec(ctx_, &plan, &vx, &s, &vc));
        return detail::from_device<CipherT>(c, n, plan.total_layer_slots, plan.total_edge_slots, prm_.m_bits, with_sigma,
                                            stream_);
    }

    // Element-wise Fp over host arrays (core/field.hpp:50-71, 209-213), one launch.
    void fp_binop(int op, const uint64_t* a_lo, const uint64_t* a_hi, const uint64_t* b_lo, const uint64_t* b_hi,
                  uint64_t* c_lo, uint64_t* c_hi, size_t n) {
        if (!n) return;
        detail::dev_array<uint64_t> d[6];
        for (auto& x : d) x.alloc(n);
        d[0].upload(a_lo, n, stream_); d[1].upload(a_hi, n, stream_);
        const size_t nb = op == PVAC_FP_SCALE ? 1 : n;
        if (op != PVAC_FP_NEG && op != PVAC_FP_INV) { d[2].upload(b_lo, nb, stream_); d[3].upload(b_hi, nb, stream_); }
        check(pvac_hip_fp_binop(ctx_, op, d[0].p, d[1].p, d[2].p, d[3].p, d[4].p, d[5].p, n));
        d[4].download(c_lo, n, stream_); d[5].download(c_hi, n, stream_);
        detail::hip_ok(hipStreamSynchronize(stream_), "sync");
    }

    // Key material of enc_value / dec_value (core/types.hpp:121-137): pk.H_digest and pk.powg_B
    // from the PubKey, prf_k and lpn_s_bits from the SecKey. Uploaded once; a different SecKey
    // under the same canon_tag replaces the device copy.
    template <class PubKeyT, class SecKeyT>
    void ensure_keys(const PubKeyT& pk, const SecKeyT& sk) {
        set_noise(pk);
        const std::vector<uint64_t> fp = key_fingerprint(sk);
        if (keys_ready_ && fp == key_fp_) return;
        if (!keys_ready_) {
            check(pvac_hip_ctx_set_H_digest(ctx_, pk.H_digest.data()));
            set_powg(pk);
        }
        check(pvac_hip_ctx_set_secret(ctx_, sk.prf_k.data(), sk.lpn_s_bits.data(), (uint32_t)pk.prm.lpn_n,
                                      (uint32_t)pk.prm.lpn_t, (uint32_t)pk.prm.lpn_tau_num,
                                      (uint32_t)pk.prm.lpn_tau_den));
        key_fp_ = fp;
        keys_ready_ = true;
    }

    // Batched enc_value (ops/encrypt.hpp:281-290, depth hint 0). Value i takes `stride`
    // (enc_caps draws_hint) consecutive words of rnd, in the reference's draw order, so a single
    // value encrypted from a replayed getrandom stream is byte-identical to the reference's; the
    // source is advanced by the whole stride. A value whose rejection sampling outruns its stride
    // (status 1, never seen in practice) is re-run with its own draws extended, prefix kept.
    // depth_hint > 0: enc_value_depth (encrypt.hpp:281-287); a value of 0 is enc_zero_depth (:293-298).
    template <class PubKeyT, class SecKeyT, class CipherT>
    std::vector<CipherT> enc_value(const PubKeyT& pk, const SecKeyT& sk, const std::vector<uint64_t>& vs,
                                   bool with_sigma, const RandomSource& rnd, int depth_hint = 0) {
        const size_t n = vs.size();
        if (!n) return {};
        ensure_keys(pk, sk);
        if (with_sigma) ensure_H(pk);
        uint32_t lpv = 0, epv = 0, stride = 0;
        check(pvac_hip_enc_caps_depth(ctx_, depth_hint, &lpv, &epv, &stride));
        std::vector<uint64_t> draws((size_t)n * stride);
        for (auto& x : draws) x = rnd();
        std::vector<uint32_t> status;
        std::vector<CipherT> out = enc_run<CipherT>(vs, &draws, stride, lpv, epv, with_sigma, status, depth_hint);
        for (uint32_t grow = stride; ; grow *= 2) {
            std::vector<size_t> redo;
            for (size_t i = 0; i < n; ++i) {
                if (status[i] == 2) throw Error(PVAC_EINVAL, "enc_value: a merged edge group cancelled (p ~ 1/p)");
                if (status[i] == 1) redo.push_back(i);
            }
            if (redo.empty()) break;
            if (grow > (1u << 20)) throw Error(PVAC_EINVAL, "enc_value: random source keeps being rejected");
            const uint32_t s2 = stride + grow;
            std::vector<uint64_t> v2(redo.size()), d2((size_t)redo.size() * s2);
            for (size_t k = 0; k < redo.size(); ++k) {
                v2[k] = vs[redo[k]];
                std::memcpy(&d2[k * s2], &draws[redo[k] * stride], (size_t)stride * 8);
                for (uint32_t j = stride; j < s2; ++j) d2[k * s2 + j] = rnd();
            }
            std::vector<uint32_t> st2;
            std::vector<CipherT> o2 = enc_run<CipherT>(v2, &d2, s2, lpv, epv, with_sigma, st2, depth_hint);
            // the redone values' draws become their prefix for a further round
            std::vector<uint64_t> nd((size_t)n * s2, 0);
            for (size_t i = 0; i < n; ++i) std::memcpy(&nd[i * s2], &draws[i * stride], (size_t)stride * 8);
            for (size_t k = 0; k < redo.size(); ++k) {
                out[redo[k]] = std::move(o2[k]);
                status[redo[k]] = st2[k];
                std::memcpy(&nd[redo[k] * s2], &d2[k * s2], (size_t)s2 * 8);
            }
            draws.swap(nd);
            stride = s2;
        }
        return out;
    }

    // ... with the draws filled on the device: value i takes `stride` words of one pvac_hip_drbg_fill.
    // A value whose rejection sampling outruns its stride (status 1) is encrypted again from fresh
    // draws of twice the stride (there is no stream to keep a prefix of).
    template <class PubKeyT, class SecKeyT, class CipherT>
    std::vector<CipherT> enc_value(const PubKeyT& pk, const SecKeyT& sk, const std::vector<uint64_t>& vs,
                                   bool with_sigma, DeviceRandom, int depth_hint = 0) {
        const size_t n = vs.size();
        if (!n) return {};
        ensure_keys(pk, sk);
        if (with_sigma) ensure_H(pk);
        uint32_t lpv = 0, epv = 0, stride = 0;
        check(pvac_hip_enc_caps_depth(ctx_, depth_hint, &lpv, &epv, &stride));
        std::vector<uint32_t> status;
        std::vector<CipherT> out = enc_run<CipherT>(vs, nullptr, stride, lpv, epv, with_sigma, status, depth_hint);
        for (;;) {
            std::vector<size_t> redo;
            std::vector<uint64_t> v2;
            for (size_t i = 0; i < n; ++i) {
                if (status[i] == 2) throw Error(PVAC_EINVAL, "enc_value: a merged edge group cancelled (p ~ 1/p)");
                if (status[i] == 1) {
                    redo.push_back(i);
                    v2.push_back(vs[i]);
                }
            }
            if (redo.empty()) break;
            if (stride > (1u << 20)) throw Error(PVAC_EINVAL, "enc_value: the draws keep being rejected");
            stride *= 2;
            std::vector<uint32_t> st2;
            std::vector<CipherT> o2 = enc_run<CipherT>(v2, nullptr, stride, lpv, epv, with_sigma, st2, depth_hint);
            for (size_t k = 0; k < redo.size(); ++k) {
                out[redo[k]] = std::move(o2[k]);
                status[redo[k]] = st2[k];
            }
        }
        return out;
    }

    // A ragged batch of encryptions (pvac_hip_enc_items): item i is enc_fp_depth(Fp{v_lo, v_hi}, hint)
    // (kind PVAC_ENC_ITEM_FP) or enc_value_depth(v_lo, hint) (PVAC_ENC_ITEM_VALUE). Item i takes
    // draws_hint[i] (pvac_hip_enc_items_caps) consecutive words of rnd, in item order: the per-value
    // stride rule of enc_value. An item whose rejection sampling outruns its words (status 1) is
    // re-run with its own draws extended, prefix kept. A plan beyond 256 pre-merge edges
    // (depth hint > 124 with the default noise Params) throws Error(PVAC_ENOSYS) before any draw.
    struct EncItem {
        uint32_t kind;
        uint64_t v_lo, v_hi;
        int depth_hint;
    };
    // words of rnd each item of enc_items takes (for a caller that replays a recorded stream)
    template <class PubKeyT>
    std::vector<uint64_t> enc_items_draws(const PubKeyT& pk, const std::vector<EncItem>& its) {
        set_noise(pk);
        const std::vector<pvac_enc_item> items = abi_items(its);
        std::vector<uint64_t> hint(its.size());
        check(pvac_hip_enc_items_caps(ctx_, items.size(), items.data(), nullptr, nullptr, hint.data()));
        return hint;
    }

    template <class PubKeyT, class SecKeyT, class CipherT>
    std::vector<CipherT> enc_items(const PubKeyT& pk, const SecKeyT& sk, const std::vector<EncItem>& its, bool with_sigma,
                                   const RandomSource& rnd) {
        const size_t n = its.size();
        if (!n) return {};
        ensure_keys(pk, sk);
        if (with_sigma) ensure_H(pk);
        const std::vector<pvac_enc_item> items = abi_items(its);
        std::vector<uint64_t> hint(n);
        uint64_t ls = 0, es = 0;
        check(pvac_hip_enc_items_caps(ctx_, n, items.data(), &ls, &es, hint.data()));
        std::vector<std::vector<uint64_t>> draws(n);
        for (size_t i = 0; i < n; ++i) {
            draws[i].resize((size_t)hint[i]);
            for (auto& x : draws[i]) x = rnd();
        }
        std::vector<CipherT> out(n);
        std::vector<size_t> todo(n);
        for (size_t i = 0; i < n; ++i) todo[i] = i;
        for (int round = 0; !todo.empty(); ++round) {
            if (round > 12) throw Error(PVAC_EINVAL, "enc_items: random source keeps being rejected");
            const size_t m = todo.size();
            std::vector<pvac_enc_item> sub(m);
            std::vector<uint64_t> flat;
            for (size_t k = 0; k < m; ++k) {
                sub[k] = items[todo[k]];
                sub[k].rnd_off = flat.size();
                sub[k].rnd_cnt = draws[todo[k]].size();
                flat.insert(flat.end(), draws[todo[k]].begin(), draws[todo[k]].end());
            }
            check(pvac_hip_enc_items_caps(ctx_, m, sub.data(), &ls, &es, nullptr));
            detail::dev_array<uint64_t> d_r(flat.size());
            d_r.upload(flat.data(), flat.size(), stream_);
            detail::batch c;
            c.alloc_index(m);
            pvac_ct_batch vc = exec_out(c, m, ls, es, sigma_words(), with_sigma);
            detail::dev_array<uint32_t> st(m);
            check(pvac_hip_enc_items(ctx_, m, sub.data(), d_r.p, flat.size(), &vc, ls, es, with_sigma ? PVAC_ENC_WITH_SIGMA : 0,
                                     st.p));
            std::vector<uint32_t> status(m);
            st.download(status.data(), m, stream_);
            std::vector<CipherT> got = detail::from_device<CipherT>(c, m, ls, es, prm_.m_bits, with_sigma, stream_);
            std::vector<size_t> redo;
            for (size_t k = 0; k < m; ++k) {
                if (status[k] == 2) throw Error(PVAC_EINVAL, "enc_items: a merged edge group cancelled (p ~ 1/p)");
                if (status[k] == 1) {
                    std::vector<uint64_t>& d = draws[todo[k]];
                    const size_t more = d.size();
                    for (size_t j = 0; j < more; ++j) d.push_back(rnd());
                    redo.push_back(todo[k]);
                } else {
                    out[todo[k]] = std::move(got[k]);
                }
            }
            todo.swap(redo);
        }
        return out;
    }

    // enc_text (utils/text.hpp:39-61) of every message in one enc_items call: per message the length
    // as a value item (hint 0), then its 15-byte blocks as bare items with hints 2, 3, ... With the
    // default noise Params a message of more than 123 blocks (1,845 bytes) needs hint 125 and throws
    // Error(PVAC_ENOSYS).
    template <class PubKeyT, class SecKeyT, class CipherT>
    std::vector<std::vector<CipherT>> enc_text(const PubKeyT& pk, const SecKeyT& sk, const std::vector<std::string>& msgs,
                                               bool with_sigma, const RandomSource& rnd) {
        std::vector<EncItem> its;
        std::vector<size_t> first{0};
        for (const std::string& m : msgs) {
            size_t nb = 0;
            std::vector<uint64_t> v(2 * (m.size() / 15 + 1));
            const int rc = pvac_text_pack((const uint8_t*)m.data(), m.size(), v.data(), v.size() / 2, &nb);
            if (rc) throw Error(rc, "pvac_text_pack");
            its.push_back(EncItem{PVAC_ENC_ITEM_VALUE, (uint64_t)m.size(), 0, 0});
            for (size_t b = 0; b < nb; ++b) its.push_back(EncItem{PVAC_ENC_ITEM_FP, v[2 * b], v[2 * b + 1], (int)(2 + b)});
            first.push_back(its.size());
        }
        std::vector<CipherT> all = enc_items<PubKeyT, SecKeyT, CipherT>(pk, sk, its, with_sigma, rnd);
        std::vector<std::vector<CipherT>> out(msgs.size());
        for (size_t m = 0; m < msgs.size(); ++m)
            out[m].assign(std::make_move_iterator(all.begin() + first[m]), std::make_move_iterator(all.begin() + first[m + 1]));
        return out;
    }

    // dec_text (utils/text.hpp:63-87) of every message: one batched dec_value, then pvac_text_unpack
    // (a length whose high word is not 0 is used as the reference uses it: the low word counts)
    template <class PubKeyT, class SecKeyT, class CipherT, class FpT>
    std::vector<std::string> dec_text(const PubKeyT& pk, const SecKeyT& sk, const std::vector<const std::vector<CipherT>*>& msgs) {
        std::vector<const CipherT*> p;
        for (const auto* m : msgs)
            for (const CipherT& c : *m) p.push_back(&c);
        const std::vector<FpT> vals = dec_value<PubKeyT, SecKeyT, CipherT, FpT>(pk, sk, p);
        std::vector<std::string> out;
        size_t at = 0;
        for (const auto* m : msgs) {
            std::vector<uint64_t> d(2 * m->size() + 2);
            for (size_t k = 0; k < m->size(); ++k) { d[2 * k] = vals[at + k].lo; d[2 * k + 1] = vals[at + k].hi; }
            at += m->size();
            std::string s(15 * m->size(), '\0');
            size_t len = 0;
            uint32_t flags = 0;
            const int rc = pvac_text_unpack(d.data(), m->size(), (uint8_t*)&s[0], s.size(), &len, &flags);
            if (rc) throw Error(rc, "pvac_text_unpack");
            s.resize(len);
            out.push_back(std::move(s));
        }
        return out;
    }

    // Batched dec_value (ops/decrypt.hpp:12-89): prf_R of every BASE layer on the device
    // (pvac_hip_base_R), then the R-tree, inverses and weighted sum (pvac_hip_dec_value).
    template <class PubKeyT, class SecKeyT, class CipherT, class FpT>
    std::vector<FpT> dec_value(const PubKeyT& pk, const SecKeyT& sk, const std::vector<const CipherT*>& cs) {
        const size_t n = cs.size();
        if (!n) return {};
        ensure_keys(pk, sk);
        detail::batch x;
        pvac_ct_batch vx = stage(cs, false, x);
        detail::dev_array<uint64_t> R(2 * (x.layers.size() ? x.layers.size() : 1)), out(2 * n);
        detail::dev_array<uint32_t> st(n);
        check(pvac_hip_base_R(ctx_, &vx, R.p));
        check(pvac_hip_dec_value(ctx_, &vx, R.p, out.p, st.p));
        std::vector<uint64_t> o(2 * n);
        out.download(o.data(), 2 * n, stream_);
        const detail::hvec<uint32_t> s = detail::d2h(st.p, n, stream_);
        std::vector<FpT> r(n);
        for (size_t i = 0; i < n; ++i) {
            if (s[i] == 1) throw Error(PVAC_EINVAL, "dec_value: layer graph has a cycle or a bad parent");
            if (s[i] == 2) throw Error(PVAC_EINVAL, "dec_value: edge references a layer or idx out of range");
            r[i].lo = o[2 * i];
            r[i].hi = o[2 * i + 1];
        }
        return r;
    }

    // pk.ubk.inv (gen_ubk_public, crypto/matrix.hpp:95-164), uploaded once per engine.
    template <class PubKeyT>
    void ensure_ubk(const PubKeyT& pk) {
        if (ubk_ready_) return;
        const std::vector<int32_t> inv(pk.ubk.inv.begin(), pk.ubk.inv.end());
        check(pvac_hip_ctx_set_ubk(ctx_, inv.data(), (uint32_t)inv.size()));
        ubk_ready_ = true;
    }

    // sigma_density (ops/encrypt.hpp:29-37) per cipher: the exact popcounts from the device, the
    // reference's long double quotient on the host.
    template <class CipherT>
    std::vector<double> sigma_density(const std::vector<const CipherT*>& cs) {
        const size_t n = cs.size();
        if (!n) return {};
        detail::batch x;
        pvac_ct_batch vx = stage(cs, true, x);
        detail::dev_array<uint64_t> ones(n);
        check(pvac_hip_sigma_popcount(ctx_, &vx, ones.p));
        const detail::hvec<uint64_t> o = detail::d2h(ones.p, n, stream_);
        std::vector<double> d(n, 0.0);
        for (size_t i = 0; i < n; ++i) {
            if (cs[i]->E.empty()) continue;
            long double total = 0;
            for (size_t k = 0; k < cs[i]->E.size(); ++k) total += prm_.m_bits;
            d[i] = (double)((long double)o[i] / total);
        }
        return d;
    }

    // ubk_apply (crypto/matrix.hpp:306-310) on copies of the ciphers.
    template <class PubKeyT, class CipherT>
    std::vector<CipherT> ubk_apply(const PubKeyT& pk, const std::vector<const CipherT*>& cs) {
        const size_t n = cs.size();
        if (!n) return {};
        ensure_ubk(pk);
        detail::batch x;
        pvac_ct_batch vx = stage(cs, true, x);
        check(pvac_hip_ubk_apply(ctx_, &vx, nullptr));
        return detail::from_device<CipherT>(x, n, x.layers.size(), x.meta.size(), prm_.m_bits, true, stream_);
    }

    // compact_edges then compact_layers (ops/encrypt.hpp:39-104).
    template <class CipherT>
    std::vector<CipherT> compact(const std::vector<const CipherT*>& cs) {
        const size_t n = cs.size();
        if (!n) return {};
        detail::batch x, c;
        pvac_ct_batch vx = stage(cs, true, x);
        pvac_ct_batch vc = plan_out(c, n);
        pvac_hip_plan plan{};
        check(pvac_hip_compact_plan(ctx_, &vx, &vc, &plan));
        vc = exec_out(c, n, plan.total_layer_slots, plan.total_edge_slots, sigma_words(), true, 1);
        check(pvac_hip_compact_exec(ctx_, &plan, &vx, &vc));
        return detail::from_device<CipherT>(c, n, plan.total_layer_slots, plan.total_edge_slots, prm_.m_bits, true,
                                            stream_);
    }

    // Batched ct_recrypt (ops/recrypt.hpp:26-41) against ek.zero_pool. The reference draws one
    // csprng_u64 per loop iteration that runs (recrypt.hpp:32), and whether iteration k runs depends
    // on draws 0..k-1 only. So the draws are taken lazily, level by level: the batch runs with the
    // words drawn so far; every cipher that wanted one more iteration than it has words for gets one
    // more word of rnd (cipher order within a level) and only those ciphers run again. A single
    // cipher therefore consumes rnd exactly as the reference consumes getrandom; a cipher that does
    // not iterate (a fresh cipher, a fresh product) is done after the first pass. iters_out
    // (optional) receives the iteration counts.
    template <class PubKeyT, class CipherT>
    std::vector<CipherT> ct_recrypt(const PubKeyT& pk, const std::vector<CipherT>& pool,
                                    const std::vector<const CipherT*>& cs, const RandomSource& rnd,
                                    std::vector<uint32_t>* iters_out = nullptr) {
        const size_t n = cs.size();
        if (!n) return {};
        ensure_ubk(pk);
        std::vector<const CipherT*> pp;
        for (const CipherT& z : pool) pp.push_back(&z);
        detail::batch p;
        const pvac_ct_batch vp = stage(pp, true, p);
        std::vector<CipherT> out(n);
        std::vector<uint32_t> iters(n, 0), drawn(n, 0);
        std::vector<uint64_t> picks(8 * n, 0);
        std::vector<size_t> pending(n);
        for (size_t i = 0; i < n; ++i) pending[i] = i;
        while (!pending.empty()) {
            const size_t m = pending.size();
            std::vector<const CipherT*> sub(m);
            std::vector<uint64_t> sub_picks(8 * m);
            for (size_t j = 0; j < m; ++j) {
                sub[j] = cs[pending[j]];
                std::memcpy(&sub_picks[8 * j], &picks[8 * pending[j]], 64);
            }
            std::vector<uint32_t> sub_iters(m, 0);
            std::vector<CipherT> sub_out = recrypt_run<CipherT>(vp, sub, sub_picks, sub_iters);
            std::vector<size_t> next;
            for (size_t j = 0; j < m; ++j) {
                const size_t i = pending[j];
                if (sub_iters[j] > drawn[i]) {   // iteration drawn[i] runs: it needs its word
                    picks[8 * i + drawn[i]++] = rnd();
                    next.push_back(i);
                } else {
                    out[i] = std::move(sub_out[j]);
                    iters[i] = sub_iters[j];
                }
            }
            pending.swap(next);
        }
        if (iters_out) *iters_out = iters;
        return out;
    }

    // commit_ct (ops/commit.hpp:12-88) per cipher under pk.H_digest and pk.canon_tag. The reference
    // hashes each edge's own e.s.nbits; a cipher here has every edge at nbits = 0 (weights only) or
    // every edge at pk.prm.m_bits, and a batch may mix the two kinds (one ABI call per kind). Any
    // other width throws: there is no host fallback.
    template <class PubKeyT, class CipherT>
    std::vector<std::array<uint8_t, 32>> commit_ct(const PubKeyT& pk, const std::vector<const CipherT*>& cs) {
        const size_t n = cs.size();
        std::vector<std::array<uint8_t, 32>> out(n);
        if (!n) return out;
        check(pvac_hip_ctx_set_H_digest(ctx_, pk.H_digest.data()));
        std::vector<size_t> ids[2];   // [0] weights only, [1] with sigma
        for (size_t i = 0; i < n; ++i) {
            const size_t nb = cs[i]->E.empty() ? 0 : cs[i]->E[0].s.nbits;
            for (const auto& e : cs[i]->E)
                if (e.s.nbits != nb) throw Error(PVAC_EINVAL, "commit_ct: a cipher's edges disagree on sigma nbits");
            if (nb != 0 && nb != (size_t)prm_.m_bits)
                throw Error(PVAC_EINVAL, "commit_ct: sigma nbits is neither 0 nor pk.prm.m_bits");
            ids[nb != 0].push_back(i);
        }
        for (int kind = 0; kind < 2; ++kind) {
            const size_t m = ids[kind].size();
            if (!m) continue;
            std::vector<const CipherT*> sub(m);
            for (size_t j = 0; j < m; ++j) sub[j] = cs[ids[kind][j]];
            detail::batch x;
            pvac_ct_batch vx = stage(sub, kind == 1, x);
            detail::dev_array<uint8_t> dig(32 * m);
            check(pvac_hip_commit_ct(ctx_, &vx, dig.p));
            const detail::hvec<uint8_t> h = detail::d2h(dig.p, 32 * m, stream_);
            for (size_t j = 0; j < m; ++j) std::memcpy(out[ids[kind][j]].data(), &h[32 * j], 32);
        }
        return out;
    }

    // pk.powg_B alone: agg_layer_gsum reads no secret key (ensure_keys uploads the same table)
    template <class PubKeyT>
    void ensure_powg(const PubKeyT& pk) {
        if (keys_ready_ || powg_ready_) return;
        set_powg(pk);
        powg_ready_ = true;
    }

    // The reference's entropy expression (utils/metrics.hpp:58-67) on 256 exact byte counts: bins in
    // order 0 .. 255, p = (double)freq / total, H -= p * log2(p) over the non-empty bins.
    static double shannon_of_counts(const uint64_t* freq) {
        uint64_t total = 0;
        for (int b = 0; b < 256; ++b) total += freq[b];
        if (total == 0) return 0.0;
        double H = 0.0;
        for (int b = 0; b < 256; ++b) {
            if (freq[b] > 0) {
                const double p = (double)freq[b] / total;
                H -= p * std::log2(p);
            }
        }
        return H;
    }

    // sigma_shannon (utils/metrics.hpp:43-68) per cipher: the exact byte counts from the device
    // (pvac_hip_sigma_bytehist), the 256 logarithms on the host. 0.0 for an empty cipher and for one
    // whose edges carry no sigma words (the reference's total == 0). The reference counts each edge's
    // own e.s.w; here a cipher has every edge at ceil(m_bits / 64) words or every edge at none, and any
    // other width throws: there is no host fallback.
    template <class CipherT>
    std::vector<double> sigma_shannon(const std::vector<const CipherT*>& cs) {
        const size_t n = cs.size();
        std::vector<double> H(n, 0.0);
        std::vector<size_t> ids;
        for (size_t i = 0; i < n; ++i) {
            if (cs[i]->E.empty()) continue;
            const size_t nw = cs[i]->E[0].s.w.size();
            for (const auto& e : cs[i]->E)
                if (e.s.w.size() != nw) throw Error(PVAC_EINVAL, "sigma_shannon: a cipher's edges disagree on sigma words");
            if (nw != 0 && nw != (size_t)sigma_words())
                throw Error(PVAC_EINVAL, "sigma_shannon: sigma rows are neither empty nor ceil(m_bits / 64) words");
            if (nw) ids.push_back(i);
        }
        const size_t m = ids.size();
        if (!m) return H;
        std::vector<const CipherT*> sub(m);
        for (size_t j = 0; j < m; ++j) sub[j] = cs[ids[j]];
        detail::batch x;
        pvac_ct_batch vx = stage(sub, true, x);
        detail::dev_array<uint64_t> hist(256 * m);
        check(pvac_hip_sigma_bytehist(ctx_, &vx, hist.p));
        const detail::hvec<uint64_t> h = detail::d2h(hist.p, 256 * m, stream_);
        for (size_t j = 0; j < m; ++j) H[ids[j]] = shannon_of_counts(&h[256 * j]);
        return H;
    }

    // agg_layer_gsum (utils/metrics.hpp:70-86) of every layer of every cipher (pvac_hip_layer_gsum).
    // An edge with idx >= B (the reference reads past pk.powg_B) throws.
    template <class PubKeyT, class CipherT, class FpT>
    std::vector<std::vector<FpT>> layer_gsums(const PubKeyT& pk, const std::vector<const CipherT*>& cs) {
        const size_t n = cs.size();
        std::vector<std::vector<FpT>> out(n);
        if (!n) return out;
        ensure_powg(pk);
        detail::batch x;
        pvac_ct_batch vx = stage(cs, false, x);
        const size_t slots = x.layers.size();
        detail::dev_array<uint64_t> g(2 * (slots ? slots : 1));
        detail::dev_array<uint32_t> st(n);
        check(pvac_hip_layer_gsum(ctx_, &vx, g.p, st.p));
        std::vector<uint32_t> s(n);
        st.download(s.data(), n, stream_);
        const detail::hvec<uint64_t> w = detail::d2h(g.p, 2 * slots, stream_);
        for (size_t i = 0; i < n; ++i) {
            if (s[i]) throw Error(PVAC_EINVAL, "agg_layer_gsum: an edge's idx is out of range");
            out[i].resize(cs[i]->L.size());
            for (size_t l = 0; l < out[i].size(); ++l) {
                out[i][l].lo = w[2 * (x.l_off[i] + l)];
                out[i][l].hi = w[2 * (x.l_off[i] + l) + 1];
            }
        }
        return out;
    }

    // ---- the device .ct codec (pvac_hip_ct_image_plan / _write / _parse)
    // The .ct file image of a resident batch (a device view, dense or capacity-padded CSR): built on
    // the device and copied to the host once; exactly the bytes pvac_ct_write gives for its used rows.
    // A view without sigma is written weights-only.
    std::vector<uint8_t> ct_image(const pvac_ct_batch& dev_view, uint32_t sigma_bits) {
        detail::dev_array<uint64_t> pos(dev_view.n + 1);
        uint64_t bytes = 0;
        check(pvac_hip_ct_image_plan(ctx_, &dev_view, sigma_bits, pos.p, &bytes));
        detail::dev_array<uint8_t> image((bytes + 15) & ~15ull);
        check(pvac_hip_ct_image_write(ctx_, &dev_view, sigma_bits, pos.p, image.p, bytes));
        std::vector<uint8_t> out(bytes);
        image.download(out.data(), bytes, stream_);
        detail::hip_ok(hipStreamSynchronize(stream_), "sync");
        return out;
    }

    // A .ct file's bytes as a resident batch that owns its arrays: the ciphers are indexed on the
    // host (offsets only), the bytes uploaded once and parsed on the device into exactly the arrays
    // pvac_ct_parse gives. Sigma rows are kept when the file carries them.
    device_batch batch_from_image(const std::vector<uint8_t>& file) {
        pvac_ct_file_info info{};
        std::vector<uint64_t> pos(64);
        int rc = pvac_ct_index(file.data(), file.size(), &info, pos.data(), pos.size());
        if (rc == PVAC_ENOMEM) {
            pos.resize(info.n_ciphers + 1);
            rc = pvac_ct_index(file.data(), file.size(), &info, pos.data(), pos.size());
        }
        if (rc) throw Error(rc, "batch_from_image: not a .ct file image");
        if (info.flags & PVAC_CT_MIXED_SIGMA) throw Error(PVAC_ENOSYS, "batch_from_image: the edges disagree on sigma nbits");
        const size_t n = info.n_ciphers;
        const bool sig = info.sigma_words != 0;
        detail::dev_array<uint8_t> image((file.size() + 15) & ~size_t(15));
        image.upload(file.data(), file.size(), stream_);
        detail::dev_array<uint64_t> dpos(n + 1);
        dpos.upload(pos.data(), n + 1, stream_);
        device_batch out;
        out.sigma_bits = info.sigma_bits;
        detail::batch& b = out.arrays;
        b.alloc_index(n);
        pvac_ct_batch v = exec_out(b, n, info.total_layers, info.total_edges, info.sigma_words, sig);
        check(pvac_hip_ct_image_parse(ctx_, image.p, file.size(), dpos.p, n, info.sigma_bits, &v, info.total_layers,
                                      info.total_edges, nullptr));
        return out;
    }

    // ---- regrouping resident batches (pvac_hip_batch_gather_plan / _exec)
    // Output cipher k = cipher pick_idx[k] of srcs[pick_src[k]], copied on the device into a batch that
    // owns its arrays (as batch_from_image's result does). pick_src empty with pick_idx given: every
    // pick comes from the one source. The sources must agree on sigma_bits (Error(PVAC_EINVAL)); the
    // result carries it, sigma rows included. Two .ct files become one in a single step:
    // batch_from_image twice, concat, ct_image.
    device_batch gather(const std::vector<const device_batch*>& srcs, const std::vector<uint32_t>& pick_src,
                        const std::vector<uint64_t>& pick_idx) {
        if (!pick_src.empty() && pick_src.size() != pick_idx.size())
            throw Error(PVAC_EINVAL, "gather: pick_src and pick_idx differ in length");
        detail::dev_array<uint32_t> ps(pick_src.size());
        detail::dev_array<uint64_t> pi(pick_idx.size());
        ps.upload(pick_src.data(), pick_src.size(), stream_);
        pi.upload(pick_idx.data(), pick_idx.size(), stream_);
        // no picks at all is the empty batch, not the concatenation: both lists stay non-null
        return gather_run(srcs, pick_idx.size(), pick_src.empty() && !pick_idx.empty() ? nullptr : ps.p, pi.p);
    }

    // the sources' ciphers in order
    device_batch concat(const std::vector<const device_batch*>& srcs) {
        uint64_t m = 0;
        for (const device_batch* s : srcs) m += s ? s->arrays.l_cnt.size() : 0;
        return gather_run(srcs, m, nullptr, nullptr);
    }

private:
    device_batch gather_run(const std::vector<const device_batch*>& srcs, uint64_t m, const uint32_t* pick_src,
                            const uint64_t* pick_idx) {
        std::vector<pvac_ct_batch> views;
        device_batch out;
        for (const device_batch* s : srcs) {
            if (!s) throw Error(PVAC_EINVAL, "gather: null source");
            if (!views.empty() && s->sigma_bits != out.sigma_bits)
                throw Error(PVAC_EINVAL, "gather: the sources disagree on sigma_bits");
            out.sigma_bits = s->sigma_bits;
            views.push_back(const_cast<device_batch*>(s)->view());
        }
        const bool sig = out.sigma_bits != 0;
        const uint32_t sw = views.empty() ? 0 : views[0].sigma_words;
        pvac_gather G{};
        G.srcs = views.data();
        G.n_src = (uint32_t)views.size();
        G.m = m;
        G.pick_src = pick_src;
        G.pick_idx = pick_idx;
        detail::batch& b = out.arrays;
        pvac_ct_batch v = plan_out(b, m);
        uint64_t tot[2] = {0, 0};
        check(pvac_hip_batch_gather_plan(ctx_, &G, &v, tot));
        v = exec_out(b, m, tot[0], tot[1], sw, sig);
        check(pvac_hip_batch_gather_exec(ctx_, &G, &v, tot[0], tot[1]));
        // the pick lists and the views die with this call: the rows must have been read by then
        detail::hip_ok(hipStreamSynchronize(stream_), "sync");
        return out;
    }

    void check(int rc) {
        if (rc) throw Error(rc, std::string("pvac_hip: ") + pvac_hip_last_error(ctx_));
    }

    template <class SecKeyT>
    static std::vector<uint64_t> key_fingerprint(const SecKeyT& sk) {
        std::vector<uint64_t> f(sk.prf_k.begin(), sk.prf_k.end());
        f.insert(f.end(), sk.lpn_s_bits.begin(), sk.lpn_s_bits.end());
        return f;
    }

    // Ciphers -> x, resident on the device (the copies are asynchronous on stream_), and its view. The
    // one flag decides whether the host image, the upload and the view carry sigma.
    template <class CipherT>
    pvac_ct_batch stage(const std::vector<const CipherT*>& cs, bool with_sigma, detail::batch& x) {
        detail::to_host(cs, sigma_words(), with_sigma, x);
        detail::upload(x, stream_, with_sigma);
        return x.view(with_sigma);
    }

    // The output batch of a plan / exec pair, in two steps around the two ABI calls. Before the plan:
    // the per-cipher arrays it fills, as the view it takes.
    static pvac_ct_batch plan_out(detail::batch& c, size_t n, uint32_t words = 0) {
        c.alloc_index(n);
        return c.plan_view(words);
    }
    // After it (or, where an operation has no plan, after alloc_index): rows at the totals, as the view
    // exec writes. min_slots = 1 where a plan may total 0 (compact, recrypt): the allocation is sized
    // for one row then, the download still takes the totals.
    static pvac_ct_batch exec_out(detail::batch& c, size_t n, uint64_t lslots, uint64_t eslots, uint32_t words,
                                  bool with_sigma, uint64_t min_slots = 0) {
        c.alloc_rows(n, std::max(lslots, min_slots), std::max(eslots, min_slots), words, with_sigma);
        return c.out_view(n, with_sigma);
    }

    template <class PubKeyT>
    void set_powg(const PubKeyT& pk) {
        std::vector<uint64_t> pg(2 * pk.powg_B.size());
        for (size_t i = 0; i < pk.powg_B.size(); ++i) { pg[2 * i] = pk.powg_B[i].lo; pg[2 * i + 1] = pk.powg_B[i].hi; }
        check(pvac_hip_ctx_set_powg(ctx_, pg.data(), (uint32_t)pk.powg_B.size()));
    }

    // plan_noise's Params fields (core/types.hpp:48-50), read on every call like the reference
    template <class PubKeyT>
    void set_noise(const PubKeyT& pk) {
        check(pvac_hip_ctx_set_noise(ctx_, (double)pk.prm.noise_entropy_bits, (double)pk.prm.tuple2_fraction,
                                     (double)pk.prm.depth_slope_bits));
    }

    static std::vector<pvac_enc_item> abi_items(const std::vector<EncItem>& its) {
        std::vector<pvac_enc_item> items(its.size());
        for (size_t i = 0; i < its.size(); ++i)
            items[i] = pvac_enc_item{its[i].v_lo, its[i].v_hi, its[i].depth_hint, its[i].kind, 0, 0};
        return items;
    }

    // the batched ct_mul's engine-owned arrays
    void release_mul() {
        mul_a_.release(); mul_b_.release(); mul_c_.release(); mul_p_.release();
        mul_nonces_.release(); mul_salts_.release(); mul_status_.release();
    }

    // one pvac_hip_ct_recrypt_plan + _exec over cs with 8 picks per cipher (vp: the uploaded pool)
    template <class CipherT>
    std::vector<CipherT> recrypt_run(const pvac_ct_batch& vp, const std::vector<const CipherT*>& cs,
                                     const std::vector<uint64_t>& picks, std::vector<uint32_t>& iters) {
        const size_t n = cs.size();
        detail::batch x, c;
        pvac_ct_batch vx = stage(cs, true, x);
        pvac_ct_batch vc = plan_out(c, n);
        pvac_hip_plan plan{};
        check(pvac_hip_ct_recrypt_plan(ctx_, &vx, &vp, &vc, &plan));
        vc = exec_out(c, n, plan.total_layer_slots, plan.total_edge_slots, sigma_words(), true, 1);
        iters.assign(n, 0);
        check(pvac_hip_ct_recrypt_exec(ctx_, &plan, &vx, &vp, picks.data(), &vc, iters.data()));
        return detail::from_device<CipherT>(c, n, plan.total_layer_slots, plan.total_edge_slots, prm_.m_bits, true,
                                            stream_);
    }

    // one pvac_hip_enc_value launch over (vs, draws) with a fixed stride; status per value
    template <class CipherT>
    // draws == nullptr: n * stride words of the device generator
    std::vector<CipherT> enc_run(const std::vector<uint64_t>& vs, const std::vector<uint64_t>* draws, uint32_t stride,
                                 uint32_t lpv, uint32_t epv, bool with_sigma, std::vector<uint32_t>& status,
                                 int depth_hint = 0) {
        const size_t n = vs.size();
        detail::dev_array<uint64_t> d_v(n), d_r(draws ? draws->size() : n * (size_t)stride);
        d_v.upload(vs.data(), n, stream_);
        if (draws) d_r.upload(draws->data(), draws->size(), stream_);
        else check(pvac_hip_drbg_fill(ctx_, d_r.p, n * (size_t)stride));
        detail::batch c;
        c.alloc_index(n);
        const uint64_t lslots = (uint64_t)n * lpv, eslots = (uint64_t)n * epv;
        pvac_ct_batch vc = exec_out(c, n, lslots, eslots, sigma_words(), with_sigma);
        detail::dev_array<uint32_t> st(n);
        check(pvac_hip_enc_value_depth(ctx_, n, d_v.p, d_r.p, stride, depth_hint, &vc,
                                       with_sigma ? PVAC_ENC_WITH_SIGMA : 0, st.p));
        status.resize(n);
        st.download(status.data(), n, stream_);
        return detail::from_device<CipherT>(c, n, lslots, eslots, prm_.m_bits, with_sigma, stream_);
    }

    pvac_hip_params prm_;
    pvac_hip_ctx* ctx_ = nullptr;
    hipStream_t stream_ = nullptr;
    bool h_ready_ = false;
    bool keys_ready_ = false;
    bool ubk_ready_ = false;
    bool powg_ready_ = false;
    Phases phases_;
    detail::pinned_batch mul_a_, mul_b_, mul_c_, mul_p_;
    detail::dev_array<uint64_t> mul_nonces_, mul_salts_;
    detail::dev_array<uint32_t> mul_status_;
    std::vector<uint64_t> key_fp_;
};

namespace detail {
template <class T, class = void>
struct has_ubk : std::false_type {};
template <class T>
struct has_ubk<T, std::void_t<decltype(std::declval<const T&>().ubk.inv)>> : std::true_type {};
}  // namespace detail

// Process-wide engines keyed by canon_tag (one public key = one context), device 0 unless
// PVAC_HIP_DEVICE is set. Contexts are not shared between threads (C ABI contract).
template <class PubKeyT>
Engine& engine_for(const PubKeyT& pk) {
    thread_local std::map<uint64_t, std::unique_ptr<Engine>> engines;
    auto it = engines.find(pk.canon_tag);
    if (it == engines.end()) {
        const char* d = std::getenv("PVAC_HIP_DEVICE");
        it = engines.emplace(pk.canon_tag, std::make_unique<Engine>(d ? std::atoi(d) : 0, Engine::params_of(pk))).first;
        // pk.ubk.inv goes up once with the engine (ubk_apply, ct_recrypt); key types without it skip this
        if constexpr (detail::has_ubk<PubKeyT>::value)
            if (!pk.ubk.inv.empty()) it->second->ensure_ubk(pk);
    }
    return *it->second;
}

// ---- drop-in single-op forms (ops/arithmetic.hpp signatures) ------------------------------
template <class PubKeyT, class CipherT>
CipherT ct_mul(const PubKeyT& pk, const CipherT& A, const CipherT& B, const RandomSource& rnd = os_random_u64) {
    return engine_for(pk).ct_mul(pk, std::vector<const CipherT*>{&A}, std::vector<const CipherT*>{&B}, true, rnd)[0];
}

template <class PubKeyT, class CipherT>
CipherT ct_add(const PubKeyT& pk, const CipherT& A, const CipherT& B) {
    return engine_for(pk).ct_add(std::vector<const CipherT*>{&A}, std::vector<const CipherT*>{&B}, false)[0];
}

template <class PubKeyT, class CipherT>
CipherT ct_sub(const PubKeyT& pk, const CipherT& A, const CipherT& B) {
    return engine_for(pk).ct_add(std::vector<const CipherT*>{&A}, std::vector<const CipherT*>{&B}, true)[0];
}

// ct_scale (ops/arithmetic.hpp:33-37): every edge weight times s.
template <class PubKeyT, class CipherT, class FpT>
CipherT ct_scale(const PubKeyT& pk, const CipherT& A, const FpT& s) {
    CipherT C = A;
    const size_t n = C.E.size();
    std::vector<uint64_t> lo(n), hi(n), slo{s.lo}, shi{s.hi};
    for (size_t i = 0; i < n; ++i) { lo[i] = C.E[i].w.lo; hi[i] = C.E[i].w.hi; }
    engine_for(pk).fp_binop(PVAC_FP_SCALE, lo.data(), hi.data(), slo.data(), shi.data(), lo.data(), hi.data(), n);
    for (size_t i = 0; i < n; ++i) { C.E[i].w.lo = lo[i]; C.E[i].w.hi = hi[i]; }
    return C;
}

// ct_neg (ops/arithmetic.hpp:39-41): ct_scale by fp_neg(fp_from_u64(1)) = p - 1.
template <class PubKeyT, class CipherT>
CipherT ct_neg(const PubKeyT& pk, const CipherT& A) {
    std::decay_t<decltype(A.E[0].w)> s{};
    s.lo = ~0ull - 1;
    s.hi = 0x7FFFFFFFFFFFFFFFull;
    return ct_scale(pk, A, s);
}

// ct_div_const (ops/arithmetic.hpp:108-110): ct_scale by fp_inv(k) (core/field.hpp:229-273; the
// inverse is unique, so the device's addition chain, PVAC_FP_INV, gives the reference's value;
// fp_inv(0) = 0 as there).
template <class PubKeyT, class CipherT, class FpT>
CipherT ct_div_const(const PubKeyT& pk, const CipherT& A, const FpT& k) {
    uint64_t lo = k.lo, hi = k.hi;
    engine_for(pk).fp_binop(PVAC_FP_INV, &lo, &hi, nullptr, nullptr, &lo, &hi, 1);
    FpT inv = k;
    inv.lo = lo;
    inv.hi = hi;
    return ct_scale(pk, A, inv);
}

// ---- batched forms ------------------------------------------------------------------------
template <class PubKeyT, class CipherT>
std::vector<CipherT> ct_mul_batch(const PubKeyT& pk, const std::vector<CipherT>& A, const std::vector<CipherT>& B,
                                  bool with_sigma = true, const RandomSource& rnd = os_random_u64) {
    std::vector<const CipherT*> a, b;
    for (auto& x : A) a.push_back(&x);
    for (auto& x : B) b.push_back(&x);
    return engine_for(pk).ct_mul(pk, a, b, with_sigma, rnd);
}

// Nonces and salts from the device generator (device_random): no per-word host work, no upload.
template <class PubKeyT, class CipherT>
std::vector<CipherT> ct_mul_batch(const PubKeyT& pk, const std::vector<CipherT>& A, const std::vector<CipherT>& B,
                                  bool with_sigma, DeviceRandom) {
    std::vector<const CipherT*> a, b;
    for (auto& x : A) a.push_back(&x);
    for (auto& x : B) b.push_back(&x);
    return engine_for(pk).ct_mul(pk, a, b, with_sigma, device_random);
}

// Multi-device batch: pairs split into contiguous ranges, one per entry of `devices` (an ordinal may
// repeat), each range on its own host thread and context. Draws from rnd stay in the one-device order:
// every pair's nonces first (pair order; their counts, 2 |A.L| |B.L| per pair, are known up front, so
// they are drawn before any device starts), then every pair's salts (pair order: range j draws its
// salts once its own weights are known and ranges < j have drawn theirs). So a replayed stream gives
// the bytes of ct_mul_batch on one device.
template <class PubKeyT, class CipherT>
std::vector<CipherT> ct_mul_batch(const PubKeyT& pk, const std::vector<CipherT>& A, const std::vector<CipherT>& B,
                                  bool with_sigma, const RandomSource& rnd, const std::vector<int>& devices) {
    if (devices.size() <= 1) {
        std::vector<const CipherT*> a, b;
        for (auto& x : A) a.push_back(&x);
        for (auto& x : B) b.push_back(&x);
        if (devices.empty()) return engine_for(pk).ct_mul(pk, a, b, with_sigma, rnd);
        Engine e(devices[0], Engine::params_of(pk));
        return e.ct_mul(pk, a, b, with_sigma, rnd);
    }
    if (A.size() != B.size()) throw Error(PVAC_EINVAL, "ct_mul_batch: |A| != |B|");
    const size_t n = A.size(), D = devices.size();
    std::vector<uint64_t> first(D + 1);
    for (size_t j = 0; j <= D; ++j) first[j] = n * j / D;
    // every nonce word, pair order
    std::vector<std::vector<uint64_t>> nonces(D);
    for (size_t j = 0; j < D; ++j)
        for (size_t i = first[j]; i < first[j + 1]; ++i)
            for (size_t k = 0; k < 2 * A[i].L.size() * B[i].L.size(); ++k) nonces[j].push_back(rnd());
    std::mutex mu;
    std::condition_variable cv;
    size_t turn = 0;   // the range whose salts are drawn next
    std::vector<std::vector<CipherT>> out(D);
    std::vector<std::exception_ptr> err(D);
    std::vector<std::thread> th;
    for (size_t j = 0; j < D; ++j)
        th.emplace_back([&, j] {
            bool my_turn = false;
            try {
                size_t pos = 0;
                // a range's source: its pre-drawn nonces, then (in range order) salts from rnd
                RandomSource src = [&]() -> uint64_t {
                    if (pos < nonces[j].size()) return nonces[j][pos++];
                    if (!my_turn) {
                        std::unique_lock<std::mutex> g(mu);
                        cv.wait(g, [&] { return turn == j; });
                        my_turn = true;
                    }
                    std::lock_guard<std::mutex> g(mu);
                    return rnd();
                };
                std::vector<const CipherT*> a, b;
                for (size_t i = first[j]; i < first[j + 1]; ++i) {
                    a.push_back(&A[i]);
                    b.push_back(&B[i]);
                }
                Engine e(devices[j], Engine::params_of(pk));
                out[j] = e.ct_mul(pk, a, b, with_sigma, src);
            } catch (...) {
                err[j] = std::current_exception();
            }
            {
                // hand the salt turn on (also when this range drew none, or failed)
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return turn == j; });
                ++turn;
            }
            cv.notify_all();
        });
    for (auto& t : th) t.join();
    for (auto& e : err)
        if (e) std::rethrow_exception(e);
    std::vector<CipherT> all;
    all.reserve(n);
    for (auto& v : out)
        for (auto& c : v) all.push_back(std::move(c));
    return all;
}

// Chains through the chain entry point (Engine::ct_mul_chain): one RandomSource per input.
template <class PubKeyT, class CipherT>
std::vector<CipherT> ct_mul_chain(const PubKeyT& pk, const std::vector<CipherT>& xs, uint32_t depth, bool with_sigma,
                                  std::vector<RandomSource>& rnds, const std::vector<int>& devices = {}) {
    std::vector<const CipherT*> x;
    for (auto& c : xs) x.push_back(&c);
    return engine_for(pk).ct_mul_chain(pk, x, depth, with_sigma, rnds, devices);
}

// ... with the chain workers' device generators: not reproducible (chunks go to workers as they come).
template <class PubKeyT, class CipherT>
std::vector<CipherT> ct_mul_chain(const PubKeyT& pk, const std::vector<CipherT>& xs, uint32_t depth, bool with_sigma,
                                  DeviceRandom, const std::vector<int>& devices = {}) {
    std::vector<const CipherT*> x;
    for (auto& c : xs) x.push_back(&c);
    return engine_for(pk).ct_mul_chain(pk, x, depth, with_sigma, device_random, devices);
}

// The reference's loop c_k = ct_mul(c_{k-1}, y_k) with a fresh operand per step (tests/test_main.cpp:
// 289-293): ys[k - 1][i] is chain i's operand at step k (depth = ys.size()).
template <class PubKeyT, class CipherT>
std::vector<CipherT> ct_mul_chain(const PubKeyT& pk, const std::vector<CipherT>& xs,
                                  const std::vector<std::vector<CipherT>>& ys, bool with_sigma,
                                  std::vector<RandomSource>& rnds, const std::vector<int>& devices = {}) {
    std::vector<const CipherT*> x;
    for (auto& c : xs) x.push_back(&c);
    std::vector<std::vector<const CipherT*>> ops(ys.size());
    for (size_t d = 0; d < ys.size(); ++d)
        for (auto& c : ys[d]) ops[d].push_back(&c);
    return engine_for(pk).ct_mul_chain(pk, x, (uint32_t)ys.size(), with_sigma, rnds, devices, 2, 16, ops);
}

template <class PubKeyT, class CipherT>
std::vector<CipherT> ct_add_batch(const PubKeyT& pk, const std::vector<CipherT>& A, const std::vector<CipherT>& B,
                                  bool negate_b = false) {
    std::vector<const CipherT*> a, b;
    for (auto& x : A) a.push_back(&x);
    for (auto& x : B) b.push_back(&x);
    return engine_for(pk).ct_add(a, b, negate_b);
}

// ---- sums of many ciphers: the fold acc = {}; acc = ct_add(pk, acc, [ct_scale(pk, x_k, s_k)]) in one call
// (sum_sq = ct_add(pk, sum_sq, ...) loops and ct_add / ct_sub / ct_scale polynomials of the reference's
// examples). Bit-exact with that fold, guard_budget and compact_layers included. INTEGRATION.md says
// when to prefer it over ct_add_batch.
template <class PubKeyT, class CipherT, class FpT>
std::vector<CipherT> ct_lincomb_batch(const PubKeyT& pk, const std::vector<CipherT>& X, const std::vector<uint64_t>& seg_off,
                                      const std::vector<uint64_t>& term, const std::vector<FpT>& scales,
                                      const std::vector<uint32_t>& flags = {}, bool with_sigma = true) {
    std::vector<const CipherT*> x;
    for (auto& c : X) x.push_back(&c);
    return engine_for(pk).ct_lincomb(x, detail::flatten_lincomb(X.size(), seg_off, term, scales, flags), with_sigma);
}

// cs[0] + cs[1] + ... (an empty vector gives the empty cipher)
template <class PubKeyT, class CipherT>
CipherT ct_sum(const PubKeyT& pk, const std::vector<CipherT>& cs, bool with_sigma = true) {
    using FpT = std::decay_t<decltype(cs[0].E[0].w)>;
    std::vector<uint64_t> term(cs.size());
    for (size_t k = 0; k < cs.size(); ++k) term[k] = k;
    return ct_lincomb_batch(pk, cs, {0, (uint64_t)cs.size()}, term, std::vector<FpT>{}, {}, with_sigma)[0];
}

// scales[0] cs[0] + scales[1] cs[1] + ...: every term goes through ct_scale, whatever its scale
template <class PubKeyT, class CipherT, class FpT>
CipherT ct_lincomb(const PubKeyT& pk, const std::vector<CipherT>& cs, const std::vector<FpT>& scales, bool with_sigma = true) {
    if (scales.size() != cs.size()) throw Error(PVAC_EINVAL, "ct_lincomb: one scale per cipher");
    std::vector<uint64_t> term(cs.size());
    for (size_t k = 0; k < cs.size(); ++k) term[k] = k;
    // no scales at all would mean "unscaled": an empty sum has nothing to scale either way
    return ct_lincomb_batch(pk, cs, {0, (uint64_t)cs.size()}, term, scales, {}, with_sigma)[0];
}

// ---- ct_recrypt and its parts (ops/recrypt.hpp, ops/encrypt.hpp:29-104, crypto/matrix.hpp:306-310)
template <class PubKeyT, class CipherT>
double sigma_density(const PubKeyT& pk, const CipherT& C) {
    return engine_for(pk).sigma_density(std::vector<const CipherT*>{&C})[0];
}

// in place, as the reference's
template <class PubKeyT, class CipherT>
void ubk_apply(const PubKeyT& pk, CipherT& C) {
    if (C.E.empty()) return;
    C = engine_for(pk).ubk_apply(pk, std::vector<const CipherT*>{&C})[0];
}

// compact_edges then compact_layers, in place: the reference's ct_recrypt always ends with the two
// together (recrypt.hpp:38-39); compact_layers alone changes nothing on the result
template <class PubKeyT, class CipherT>
void compact_edges(const PubKeyT& pk, CipherT& C) {
    C = engine_for(pk).compact(std::vector<const CipherT*>{&C})[0];
}

template <class PubKeyT, class EvalKeyT, class CipherT>
CipherT ct_recrypt(const PubKeyT& pk, const EvalKeyT& ek, const CipherT& in, const RandomSource& rnd = os_random_u64) {
    if (ek.zero_pool.empty() || in.E.empty()) return in;   // recrypt.hpp:27
    return engine_for(pk).ct_recrypt(pk, ek.zero_pool, std::vector<const CipherT*>{&in}, rnd)[0];
}

template <class PubKeyT, class EvalKeyT, class CipherT>
std::vector<CipherT> ct_recrypt_batch(const PubKeyT& pk, const EvalKeyT& ek, const std::vector<CipherT>& in,
                                      const RandomSource& rnd = os_random_u64,
                                      std::vector<uint32_t>* iters_out = nullptr) {
    std::vector<const CipherT*> p;
    for (auto& x : in) p.push_back(&x);
    return engine_for(pk).ct_recrypt(pk, ek.zero_pool, p, rnd, iters_out);
}

// ---- commit_ct (ops/commit.hpp:12-88) --------------------------------------------------------
template <class PubKeyT, class CipherT>
std::array<uint8_t, 32> commit_ct(const PubKeyT& pk, const CipherT& C) {
    return engine_for(pk).commit_ct(pk, std::vector<const CipherT*>{&C})[0];
}

// every cipher's commitment; ciphers with sigma (nbits = pk.prm.m_bits) and without (nbits = 0) may mix
template <class PubKeyT, class CipherT>
std::vector<std::array<uint8_t, 32>> commit_ct_batch(const PubKeyT& pk, const std::vector<CipherT>& cs) {
    std::vector<const CipherT*> p;
    for (auto& x : cs) p.push_back(&x);
    return engine_for(pk).commit_ct(pk, p);
}

// ---- metrics (utils/metrics.hpp) --------------------------------------------------------------
// sigma_shannon (metrics.hpp:43-68): the reference's signature has no PubKey; the engine is found by it
template <class PubKeyT, class CipherT>
double sigma_shannon(const PubKeyT& pk, const CipherT& C) {
    return engine_for(pk).sigma_shannon(std::vector<const CipherT*>{&C})[0];
}

template <class PubKeyT, class CipherT>
std::vector<double> sigma_shannon_batch(const PubKeyT& pk, const std::vector<CipherT>& cs) {
    std::vector<const CipherT*> p;
    for (auto& x : cs) p.push_back(&x);
    return engine_for(pk).sigma_shannon(p);
}

// every layer's agg_layer_gsum (metrics.hpp:70-86) of every cipher: out[i][l] = agg_layer_gsum(pk, cs[i], l)
template <class FpT, class PubKeyT, class CipherT>
std::vector<std::vector<FpT>> layer_gsums_batch(const PubKeyT& pk, const std::vector<CipherT>& cs) {
    std::vector<const CipherT*> p;
    for (auto& x : cs) p.push_back(&x);
    return engine_for(pk).template layer_gsums<PubKeyT, CipherT, FpT>(pk, p);
}

// agg_layer_gsum(pk, X, lid): a layer id no layer of X carries sums no edge the batched form reports,
// so it gives what the reference's loop gives for it when no edge names it: fp_from_u64(0)
template <class FpT, class PubKeyT, class CipherT>
FpT agg_layer_gsum(const PubKeyT& pk, const CipherT& X, uint32_t lid) {
    FpT zero{};
    zero.lo = 0;
    zero.hi = 0;
    if (lid >= X.L.size()) return zero;
    return engine_for(pk).template layer_gsums<PubKeyT, CipherT, FpT>(pk, std::vector<const CipherT*>{&X})[0][lid];
}

// dump_metrics (metrics.hpp:13-41): one CSV row per call appended to pvac_metrics.csv in the working
// directory, the header line once per process (before the first row, as the reference writes it on
// every first call of a process), the density from sigma_density above with six fixed decimals.
namespace detail {
struct metrics_csv {   // one per process, whatever types dump_metrics is instantiated on
    std::ofstream f;
    bool ready = false;
};
inline metrics_csv& metrics_csv_file() {
    static metrics_csv m;
    return m;
}
}  // namespace detail

template <class PubKeyT, class CipherT, class FpT>
void dump_metrics(const PubKeyT& pk, const char* tag, const CipherT& C, const FpT& val) {
    detail::metrics_csv& m = detail::metrics_csv_file();
    if (!m.ready) {
        m.f.open("pvac_metrics.csv", std::ios::app);
        if (!m.f) return;
        m.f << "tag,edges,layers,sigma_density,value_lo,value_hi\n";
        m.ready = true;
    }
    const double density = sigma_density(pk, C);
    m.f << tag << ',' << C.E.size() << ',' << C.L.size() << ',' << std::fixed << std::setprecision(6) << density << ','
        << val.lo << ',' << val.hi << "\n";
    m.f.flush();   // a reader in the same process sees the row (the reference leaves it to the stream's destructor)
}

// ---- encryption / decryption (ops/encrypt.hpp:289, ops/decrypt.hpp:62) --------------------
template <class CipherT, class PubKeyT, class SecKeyT>
CipherT enc_value(const PubKeyT& pk, const SecKeyT& sk, uint64_t v, const RandomSource& rnd = os_random_u64) {
    return engine_for(pk).template enc_value<PubKeyT, SecKeyT, CipherT>(pk, sk, std::vector<uint64_t>{v}, true, rnd)[0];
}

// enc_value_depth / enc_zero_depth (ops/encrypt.hpp:281-287, 293-298): the noise plan of depth_hint
template <class CipherT, class PubKeyT, class SecKeyT>
CipherT enc_value_depth(const PubKeyT& pk, const SecKeyT& sk, uint64_t v, int depth_hint,
                        const RandomSource& rnd = os_random_u64) {
    return engine_for(pk).template enc_value<PubKeyT, SecKeyT, CipherT>(pk, sk, std::vector<uint64_t>{v}, true, rnd,
                                                                         depth_hint)[0];
}

template <class CipherT, class PubKeyT, class SecKeyT>
CipherT enc_zero_depth(const PubKeyT& pk, const SecKeyT& sk, int depth_hint, const RandomSource& rnd = os_random_u64) {
    return enc_value_depth<CipherT>(pk, sk, 0, depth_hint, rnd);
}

// make_evalkey (ops/recrypt.hpp:12-19): pool_size enc_zero_depth ciphers, then enc_value(1), in the
// reference's draw order
template <class EvalKeyT, class PubKeyT, class SecKeyT>
EvalKeyT make_evalkey(const PubKeyT& pk, const SecKeyT& sk, size_t pool_size, int depth_hint,
                      const RandomSource& rnd = os_random_u64) {
    using CipherT = std::decay_t<decltype(std::declval<EvalKeyT&>().enc_one)>;
    EvalKeyT ek;
    ek.zero_pool.reserve(pool_size);
    for (size_t i = 0; i < pool_size; ++i) ek.zero_pool.push_back(enc_zero_depth<CipherT>(pk, sk, depth_hint, rnd));
    ek.enc_one = enc_value<CipherT>(pk, sk, 1, rnd);
    return ek;
}

template <class CipherT, class PubKeyT, class SecKeyT>
std::vector<CipherT> enc_value_batch(const PubKeyT& pk, const SecKeyT& sk, const std::vector<uint64_t>& vs,
                                     bool with_sigma = true, const RandomSource& rnd = os_random_u64) {
    return engine_for(pk).template enc_value<PubKeyT, SecKeyT, CipherT>(pk, sk, vs, with_sigma, rnd);
}

template <class CipherT, class PubKeyT, class SecKeyT>
std::vector<CipherT> enc_value_batch(const PubKeyT& pk, const SecKeyT& sk, const std::vector<uint64_t>& vs,
                                     bool with_sigma, DeviceRandom) {
    return engine_for(pk).template enc_value<PubKeyT, SecKeyT, CipherT>(pk, sk, vs, with_sigma, device_random);
}

template <class PubKeyT, class SecKeyT, class CipherT>
auto dec_value(const PubKeyT& pk, const SecKeyT& sk, const CipherT& C) {
    using FpT = std::decay_t<decltype(C.E[0].w)>;
    return engine_for(pk).template dec_value<PubKeyT, SecKeyT, CipherT, FpT>(pk, sk, std::vector<const CipherT*>{&C})[0];
}

template <class PubKeyT, class SecKeyT, class CipherT>
auto dec_value_batch(const PubKeyT& pk, const SecKeyT& sk, const std::vector<CipherT>& cs) {
    using FpT = std::decay_t<decltype(cs[0].E[0].w)>;
    std::vector<const CipherT*> p;
    for (auto& x : cs) p.push_back(&x);
    return engine_for(pk).template dec_value<PubKeyT, SecKeyT, CipherT, FpT>(pk, sk, p);
}

// ---- bare enc_fp_depth and text (ops/encrypt.hpp:162-258, utils/text.hpp:39-87) ------------
// enc_fp_depth: one BASE layer, no mask; v's two words go to the equations as given.
template <class CipherT, class PubKeyT, class SecKeyT, class FpT>
CipherT enc_fp_depth(const PubKeyT& pk, const SecKeyT& sk, const FpT& v, int depth_hint,
                     const RandomSource& rnd = os_random_u64) {
    return engine_for(pk).template enc_items<PubKeyT, SecKeyT, CipherT>(
        pk, sk, {Engine::EncItem{PVAC_ENC_ITEM_FP, v.lo, v.hi, depth_hint}}, true, rnd)[0];
}

// enc_text: the length, then one cipher per 15-byte block with depth hints 2, 3, ... At the default plan
// limit more than 123 blocks (1,845 bytes) under the default noise Params throw Error(PVAC_ENOSYS); raise
// it with engine_for(pk).set_enc_plan_limit(n) (hint 2 + b needs about 2 (2 + b) + 8 edges) and longer
// messages run on the wide route. enc_fp_depth, enc_value_depth, enc_zero_depth and make_evalkey follow
// the same limit.
template <class CipherT, class PubKeyT, class SecKeyT>
std::vector<std::vector<CipherT>> enc_text_batch(const PubKeyT& pk, const SecKeyT& sk, const std::vector<std::string>& msgs,
                                                 bool with_sigma = true, const RandomSource& rnd = os_random_u64) {
    return engine_for(pk).template enc_text<PubKeyT, SecKeyT, CipherT>(pk, sk, msgs, with_sigma, rnd);
}

template <class CipherT, class PubKeyT, class SecKeyT>
std::vector<CipherT> enc_text(const PubKeyT& pk, const SecKeyT& sk, const std::string& msg,
                              const RandomSource& rnd = os_random_u64) {
    return std::move(enc_text_batch<CipherT>(pk, sk, std::vector<std::string>{msg}, true, rnd)[0]);
}

template <class PubKeyT, class SecKeyT, class CipherT>
std::vector<std::string> dec_text_batch(const PubKeyT& pk, const SecKeyT& sk, const std::vector<std::vector<CipherT>>& msgs) {
    using FpT = std::decay_t<decltype(std::declval<CipherT&>().E[0].w)>;
    std::vector<const std::vector<CipherT>*> p;
    for (const auto& m : msgs) p.push_back(&m);
    return engine_for(pk).template dec_text<PubKeyT, SecKeyT, CipherT, FpT>(pk, sk, p);
}

template <class PubKeyT, class SecKeyT, class CipherT>
std::string dec_text(const PubKeyT& pk, const SecKeyT& sk, const std::vector<CipherT>& cts) {
    using FpT = std::decay_t<decltype(std::declval<CipherT&>().E[0].w)>;
    return engine_for(pk).template dec_text<PubKeyT, SecKeyT, CipherT, FpT>(
        pk, sk, std::vector<const std::vector<CipherT>*>{&cts})[0];
}

// ---- .ct files (the reference's tests/add.cpp:22-155 format) through the native codec ------
// Layers of PROD rule come back with zero seeds (the format stores none); sigmas come back as
// stored (nbits 0 and no words when the file carries none).
template <class CipherT>
std::vector<CipherT> load_cts_bytes(const std::vector<uint8_t>& buf) {
    pvac_ct_file_info info{};
    int rc = pvac_ct_scan(buf.data(), buf.size(), &info);
    if (rc) throw Error(rc, "load_cts: malformed .ct image");
    if (info.flags & PVAC_CT_MIXED_SIGMA) throw Error(PVAC_ENOSYS, "load_cts: edges disagree on sigma nbits");
    const size_t n = info.n_ciphers, nl = info.total_layers, ne = info.total_edges;
    const uint32_t sw = info.sigma_words;
    std::vector<uint64_t> l_off(n), l_cnt(n), e_off(n), e_cnt(n), meta(ne), w_lo(ne), w_hi(ne), sig(ne * sw);
    std::vector<pvac_layer> layers(nl);
    pvac_ct_batch X{};
    X.n = n; X.l_off = l_off.data(); X.l_cnt = l_cnt.data(); X.layers = layers.data();
    X.e_off = e_off.data(); X.e_cnt = e_cnt.data(); X.meta = meta.data(); X.w_lo = w_lo.data(); X.w_hi = w_hi.data();
    X.sigma = sw ? sig.data() : nullptr;
    X.sigma_words = sw;
    rc = pvac_ct_parse(buf.data(), buf.size(), &X, 0);
    if (rc) throw Error(rc, "load_cts: parse failed");
    std::vector<CipherT> out(n);
    for (size_t i = 0; i < n; ++i) {
        CipherT& C = out[i];
        C.L.resize(l_cnt[i]);
        for (size_t l = 0; l < l_cnt[i]; ++l) {
            const pvac_layer& y = layers[l_off[i] + l];
            auto& L = C.L[l];
            L.rule = static_cast<decltype(L.rule)>(y.rule);
            L.pa = y.pa; L.pb = y.pb;
            L.seed.ztag = y.ztag; L.seed.nonce.lo = y.nonce_lo; L.seed.nonce.hi = y.nonce_hi;
        }
        C.E.resize(e_cnt[i]);
        for (size_t k = 0; k < e_cnt[i]; ++k) {
            const size_t e = e_off[i] + k;
            auto& E = C.E[k];
            E.layer_id = (uint32_t)meta[e];
            E.idx = (uint16_t)(meta[e] >> 32);
            E.ch = (uint8_t)(meta[e] >> 48);
            E.w.lo = w_lo[e]; E.w.hi = w_hi[e];
            E.s.nbits = info.sigma_bits;
            E.s.w.assign(sig.begin() + e * sw, sig.begin() + (e + 1) * sw);
        }
    }
    return out;
}

// Every edge's sigma is written with nbits = sigma_bits (the reference writes m_bits = 8192).
template <class CipherT>
std::vector<uint8_t> save_cts_bytes(const std::vector<CipherT>& cs, uint32_t sigma_bits = 8192) {
    const uint32_t sw = (sigma_bits + 63) / 64;
    std::vector<const CipherT*> p;
    for (auto& x : cs) p.push_back(&x);
    detail::batch b;
    detail::to_host(p, sw, true, b);
    pvac_ct_batch X{};
    X.n = cs.size(); X.l_off = b.l_off.data(); X.l_cnt = b.l_cnt.data(); X.layers = b.layers.data();
    X.e_off = b.e_off.data(); X.e_cnt = b.e_cnt.data(); X.meta = b.meta.data();
    X.w_lo = b.w_lo.data(); X.w_hi = b.w_hi.data();
    X.sigma = b.sigma.data();
    X.sigma_words = sw;
    uint64_t bytes = 0, written = 0;
    int rc = pvac_ct_serialized_size(&X, sigma_bits, &bytes);
    if (rc) throw Error(rc, "save_cts: size");
    std::vector<uint8_t> out(bytes);
    rc = pvac_ct_write(&X, sigma_bits, out.data(), out.size(), &written, 0);
    if (rc || written != bytes) throw Error(rc ? rc : PVAC_EINVAL, "save_cts: write");
    return out;
}

}  // namespace pvac_hip

#endif  // PVAC_HIP_HPP
