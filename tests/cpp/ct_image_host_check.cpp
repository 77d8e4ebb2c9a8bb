// ct_image_host_check.cpp — csrc/ct_image.hpp (the geometry, stream words, layer bytes and parse
// validation the device .ct codec's kernels run) instantiated on the host, without a GPU:
//   ct_image_host_check [<file.ct>] ...
// every file is rebuilt granule by granule by the shared functions and must equal its bytes, and every
// cipher of it must validate with the counts the host parser read; then the alignment sweep (48
// ciphers, 0..15 layers, 0..17 edges, seven sigma settings) is rebuilt against pvac_ct_write; then the
// validation is run on malformed spans, each of which must yield status 1. Image buffers are heap
// blocks of exactly the rounded length, so ASan sees any read past it. Built as a stand-alone host
// program with ASan + UBSan (tests/test_codec_image_host.py).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "ct_image.hpp"

using namespace pvhip;

static int g_checks = 0;
#define MUST(cond, ...)                                                        \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);          \
            std::fprintf(stderr, __VA_ARGS__);                                 \
            std::fprintf(stderr, "\n");                                        \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

struct host_batch {
    std::vector<uint64_t> l_off, l_cnt, e_off, e_cnt, meta, w_lo, w_hi, sigma_store;
    std::vector<pvac_layer> layers;
    pvac_ct_batch X{};
    void bind(uint64_t n, uint32_t sigma_words, bool with_sigma, size_t sigma_shift_words = 0) {
        X.n = n;
        X.l_off = l_off.data();
        X.l_cnt = l_cnt.data();
        X.e_off = e_off.data();
        X.e_cnt = e_cnt.data();
        X.layers = layers.data();
        X.meta = meta.data();
        X.w_lo = w_lo.data();
        X.w_hi = w_hi.data();
        X.sigma = with_sigma ? sigma_store.data() + sigma_shift_words : nullptr;
        X.sigma_words = sigma_words;
    }
};

// the image of X by the shared functions alone, in a buffer of the rounded length pre-filled with 0xA5
static std::vector<uint8_t> rebuild(const pvac_ct_batch& X, uint32_t sigma_bits, std::vector<uint64_t>& pos) {
    const ct_geom g = ct_geom_of(X.sigma ? sigma_bits : 0u);
    pos.assign(X.n + 1, 0);
    pos[0] = kCtFileHdr;
    for (uint64_t i = 0; i < X.n; ++i) {
        uint32_t bad = 0;
        uint64_t b = 0;
        for (uint64_t sub = 0; sub < 8; ++sub) b += ct_layer_bytes_sum(X.layers + X.l_off[i], sub, X.l_cnt[i], 8, &bad);
        MUST(bad == 0, "rule >= 256");
        pos[i + 1] = pos[i] + kCtCipherHdr + b + X.e_cnt[i] * g.eb();
    }
    const uint64_t len = pos[X.n];
    std::vector<uint8_t> out((len + 15) & ~15ull, 0xA5);
    const uint32_t hdr[4] = {kCtMagic, kCtVersion, (uint32_t)X.n, (uint32_t)(X.n >> 32)};
    std::memcpy(out.data(), hdr, 16);
    for (uint64_t i = 0; i < X.n; ++i) {
        const uint32_t cnt[2] = {(uint32_t)X.l_cnt[i], (uint32_t)X.e_cnt[i]};
        std::memcpy(out.data() + pos[i], cnt, 8);
        uint64_t off = pos[i] + kCtCipherHdr;
        for (uint64_t l = 0; l < X.l_cnt[i]; ++l) {
            const pvac_layer& y = X.layers[X.l_off[i] + l];
            for (uint32_t k = 0; k < ct_layer_bytes(y.rule); ++k) out[off++] = ct_layer_byte(y, k);
        }
        const uint64_t E = X.e_cnt[i], ee = pos[i + 1], es = ee - E * g.eb();
        MUST(off == es, "cipher %" PRIu64 ": layers end at %" PRIu64 ", edges start at %" PRIu64, i, off, es);
        const ct_edge_view v = ct_edge_view_of(X, i, g);
        for (uint64_t a = es & ~15ull; a < ee; a += 16) {
            uint32_t w[4];
            ct_edge_granule(v, g, E, es, a, w);
            for (uint64_t b = (a < es ? es : a); b < a + 16 && b < ee; ++b) out[b] = (uint8_t)(w[(b - a) >> 2] >> (8 * (b & 3)));
        }
    }
    return out;
}

// an image as the device sees it: exactly the rounded length on the heap
struct image_block {
    std::unique_ptr<uint32_t[]> words;
    uint64_t len;
    image_block(const uint8_t* bytes, uint64_t n) : words(new uint32_t[(n + 15) / 16 * 4]), len(n) {
        std::memset(words.get(), 0xA5, (n + 15) / 16 * 16);
        std::memcpy(words.get(), bytes, n);
    }
    uint8_t* bytes() { return (uint8_t*)words.get(); }
};

static void check_against(const std::vector<uint8_t>& expect, const pvac_ct_batch& X, uint32_t sigma_bits, const char* what) {
    std::vector<uint64_t> pos;
    const std::vector<uint8_t> got = rebuild(X, sigma_bits, pos);
    MUST(pos[X.n] == expect.size(), "%s: %" PRIu64 " bytes planned, %zu expected", what, pos[X.n], expect.size());
    MUST(std::memcmp(got.data(), expect.data(), expect.size()) == 0, "%s: rebuilt image differs", what);
    for (size_t k = expect.size(); k < got.size(); ++k) MUST(got[k] == 0xA5, "%s: byte %zu past the image was written", what, k);
    // pvac_ct_index agrees with the planned offsets, and every cipher validates with the batch's counts
    pvac_ct_file_info info{};
    std::vector<uint64_t> ipos(X.n + 1);
    MUST(pvac_ct_index(expect.data(), expect.size(), &info, ipos.data(), ipos.size()) == PVAC_OK, "%s: pvac_ct_index", what);
    MUST(ipos == pos, "%s: pvac_ct_index offsets differ from the plan's", what);
    image_block img(expect.data(), expect.size());
    const ct_geom g = ct_geom_of(info.sigma_bits);
    for (uint64_t i = 0; i < X.n; ++i) {
        uint64_t nL = 0, nE = 0;
        MUST(ct_parse_validate(img.words.get(), img.len, pos.data(), X.n, i, g, &nL, &nE) == 0, "%s: cipher %" PRIu64 " refused", what, i);
        MUST(nL == X.l_cnt[i] && nE == X.e_cnt[i], "%s: cipher %" PRIu64 " counts", what, i);
    }
}

static void check_file(const char* path) {
    std::ifstream f(path, std::ios::binary);
    MUST((bool)f, "cannot open %s", path);
    const std::vector<uint8_t> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    pvac_ct_file_info info{};
    MUST(pvac_ct_scan(buf.data(), buf.size(), &info) == PVAC_OK, "%s: scan", path);
    host_batch h;
    const uint64_t n = info.n_ciphers;
    h.l_off.resize(n + 1);
    h.l_cnt.resize(n + 1);
    h.e_off.resize(n + 1);
    h.e_cnt.resize(n + 1);
    h.layers.resize(info.total_layers + 1);
    h.meta.resize(info.total_edges + 1);
    h.w_lo.resize(info.total_edges + 1);
    h.w_hi.resize(info.total_edges + 1);
    h.sigma_store.resize((info.total_edges + 1) * (uint64_t)info.sigma_words + 1);
    h.bind(n, info.sigma_words, info.sigma_words != 0);
    MUST(pvac_ct_parse(buf.data(), buf.size(), &h.X, 1) == PVAC_OK, "%s: parse", path);
    check_against(buf, h.X, info.sigma_bits, path);
}

static uint64_t g_seed = 0x5EED0C0DEull;
static uint64_t rnd() {
    uint64_t z = (g_seed += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

// the alignment sweep: cipher k has k mod 16 layers (rules cycling BASE, PROD, 2) and
// [0, 1, 2, 3, 5, 17][k mod 6] edges
static void make_sweep(host_batch& h, uint32_t sigma_words, bool with_sigma, size_t shift) {
    static const uint32_t kEdges[6] = {0, 1, 2, 3, 5, 17};
    const uint64_t n = 48;
    uint64_t lo = 0, eo = 0;
    for (uint64_t k = 0; k < n; ++k) {
        h.l_off.push_back(lo);
        h.l_cnt.push_back(k % 16);
        h.e_off.push_back(eo);
        h.e_cnt.push_back(kEdges[k % 6]);
        for (uint64_t l = 0; l < k % 16; ++l) {
            pvac_layer y{};
            y.rule = (uint32_t)(l % 3 == 2 ? 2 : l % 3);
            y.pa = (uint32_t)rnd();
            y.pb = (uint32_t)rnd();
            y.ztag = rnd();
            y.nonce_lo = rnd();
            y.nonce_hi = rnd();
            h.layers.push_back(y);
        }
        for (uint32_t e = 0; e < kEdges[k % 6]; ++e) {
            h.meta.push_back(rnd());   // the top byte is set: the writer must drop it
            h.w_lo.push_back(rnd());
            h.w_hi.push_back(rnd());
        }
        lo += k % 16;
        eo += kEdges[k % 6];
    }
    h.layers.push_back(pvac_layer{});
    h.sigma_store.resize(eo * sigma_words + shift + 1);
    for (auto& w : h.sigma_store) w = rnd();
    h.bind(n, sigma_words, with_sigma, shift);
}

static std::vector<uint8_t> host_write(const pvac_ct_batch& X, uint32_t sigma_bits) {
    uint64_t bytes = 0, wrote = 0;
    MUST(pvac_ct_serialized_size(&X, sigma_bits, &bytes) == PVAC_OK, "serialized_size");
    std::vector<uint8_t> out(bytes);
    MUST(pvac_ct_write(&X, sigma_bits, out.data(), out.size(), &wrote, 1) == PVAC_OK && wrote == bytes, "pvac_ct_write");
    return out;
}

static void check_sweep() {
    struct setting { uint32_t bits, words; bool sigma; size_t shift; };
    const setting settings[] = {{0, 128, false, 0}, {64, 1, true, 0},     {100, 2, true, 0},   {8191, 128, true, 0},
                                {8192, 128, true, 0}, {8192, 130, true, 0}, {8192, 128, true, 1}};
    for (const setting& s : settings) {
        host_batch h;
        make_sweep(h, s.words, s.sigma, s.shift);
        const std::vector<uint8_t> expect = host_write(h.X, s.bits);
        // the recipe reaches every alignment: cipher starts and edge-region starts cover all 16 residues
        std::vector<uint64_t> pos;
        rebuild(h.X, s.bits, pos);
        const ct_geom g = ct_geom_of(s.sigma ? s.bits : 0);
        uint32_t starts = 0, regions = 0;
        for (uint64_t i = 0; i < h.X.n; ++i) {
            starts |= 1u << (pos[i] & 15);
            regions |= 1u << ((pos[i + 1] - h.X.e_cnt[i] * g.eb()) & 15);
        }
        MUST(starts == 0xFFFF && regions == 0xFFFF, "sweep bits %u: residues %04x / %04x", s.bits, starts, regions);
        char what[64];
        std::snprintf(what, sizeof what, "sweep bits %u words %u shift %zu", s.bits, s.words, s.shift);
        check_against(expect, h.X, s.bits, what);
    }
}

// every malformed span must be refused (status 1) without a read outside the rounded image
static void check_malformed() {
    host_batch h;
    make_sweep(h, 2, true, 0);
    const uint32_t bits = 100;
    const std::vector<uint8_t> good = host_write(h.X, bits);
    std::vector<uint64_t> pos;
    rebuild(h.X, bits, pos);
    const ct_geom g = ct_geom_of(bits);
    const uint64_t n = h.X.n, i = 29;   // 13 layers, 17 edges, ciphers on both sides
    uint64_t nL, nE;
    auto status = [&](image_block& img, const std::vector<uint64_t>& p, uint64_t c) {
        return ct_parse_validate(img.words.get(), img.len, p.data(), n, c, g, &nL, &nE);
    };
    {
        image_block img(good.data(), good.size());
        for (uint64_t c = 0; c < n; ++c) MUST(status(img, pos, c) == 0, "the well-formed image is refused at %" PRIu64, c);
        std::vector<uint64_t> p = pos;
        p[i + 1] = p[i] - 1;   // pos decreasing
        MUST(status(img, p, i) == 1 && nL == 0 && nE == 0, "decreasing pos accepted");
        p = pos;
        p[i + 1] = good.size() + 5;   // pos past len
        MUST(status(img, p, i) == 1, "pos past len accepted");
        MUST(status(img, p, i + 1) == 1, "a start past len accepted");
        p = pos;
        p[n] = good.size() - 1;   // pos[n] != len
        MUST(status(img, p, n - 1) == 1, "pos[n] != len accepted");
        p = pos;
        p[0] = 17;
        MUST(status(img, p, 0) == 1, "pos[0] != 16 accepted");
        p = pos;
        p[i + 1] = pos[i + 1] - 1;   // the layer walk now ends one byte late
        MUST(status(img, p, i) == 1, "a walk ending one byte late accepted");
        p[i + 1] = pos[i + 1] + 1;   // ... and one byte early
        MUST(status(img, p, i) == 1, "a walk ending one byte early accepted");
        p[i + 1] = pos[i] + 7;       // a span that cannot hold the count words
        MUST(status(img, p, i) == 1, "a 7-byte span accepted");
    }
    auto with_counts = [&](uint32_t L, uint32_t E) {
        std::vector<uint8_t> bad = good;
        std::memcpy(bad.data() + pos[i], &L, 4);
        std::memcpy(bad.data() + pos[i] + 4, &E, 4);
        return bad;
    };
    {
        const std::vector<uint8_t> bad = with_counts(13, 0xFFFFFFFFu);   // |E| eb larger than the span
        image_block img(bad.data(), bad.size());
        MUST(status(img, pos, i) == 1, "|E| = 2^32 - 1 accepted");
        const std::vector<uint8_t> bad2 = with_counts(13, 18);
        image_block img2(bad2.data(), bad2.size());
        MUST(status(img2, pos, i) == 1, "|E| one too many accepted");
    }
    {
        const std::vector<uint8_t> bad = with_counts(0xFFFFFFFFu, 17);   // |L| = 2^32 - 1
        image_block img(bad.data(), bad.size());
        MUST(status(img, pos, i) == 1, "|L| = 2^32 - 1 accepted");
        const std::vector<uint8_t> bad2 = with_counts(12, 17);
        image_block img2(bad2.data(), bad2.size());
        MUST(status(img2, pos, i) == 1, "|L| one too few accepted");
    }
    {   // the last cipher with its counts enlarged: the walk must stop at the image's end
        std::vector<uint8_t> bad = good;
        const uint32_t L = 1000;
        std::memcpy(bad.data() + pos[n - 1], &L, 4);
        image_block img(bad.data(), bad.size());
        MUST(status(img, pos, n - 1) == 1, "a walk past the image accepted");
    }
}

int main(int argc, char** argv) {
    for (int k = 1; k < argc; ++k) check_file(argv[k]);
    check_sweep();
    check_malformed();
    std::printf("ct_image_host_check: ok (%d files, %d checks)\n", argc - 1, g_checks);
    return 0;
}
