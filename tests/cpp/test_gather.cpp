// test_gather.cpp — regrouping resident batches through the C++ adapter (include/pvac_hip.hpp). Runs on the
// GPU box:
//   test_gather <file.ct> ...              files that agree on sigma nbits
//   test_gather --mismatch <a.ct> <b.ct>   two files that do not
// Every file goes through Engine::batch_from_image; Engine::concat of all of them and an Engine::gather
// with a pick list (reversed order, a repeat, one source left out when there are several) go through
// Engine::ct_image and must be the bytes pvac_ct_write gives for the same regrouping of the host-parsed
// ciphers. Exit 0 = every check passed; failures abort with a message.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "pvac_hip.hpp"

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

static std::vector<uint8_t> slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    MUST(f.good(), "open %s", p.c_str());
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// every file parsed on the host into one set of arrays; cipher c of file f is entry first[f] + c
struct host_pool {
    std::vector<uint64_t> l_off, l_cnt, e_off, e_cnt, meta, w_lo, w_hi, sigma;
    std::vector<pvac_layer> layers;
    std::vector<size_t> first;
    uint32_t sigma_bits = 0, sigma_words = 0;

    void add(const std::vector<uint8_t>& file) {
        pvac_ct_file_info info{};
        MUST(pvac_ct_scan(file.data(), file.size(), &info) == PVAC_OK, "scan");
        if (first.empty()) {
            sigma_bits = info.sigma_bits;
            sigma_words = info.sigma_words;
        }
        MUST(info.sigma_bits == sigma_bits, "the files disagree on sigma nbits");
        const size_t n = info.n_ciphers, nl = info.total_layers, ne = info.total_edges, c0 = l_cnt.size(), l0 = layers.size(),
                     e0 = meta.size();
        first.push_back(c0);
        for (auto* v : {&l_off, &l_cnt, &e_off, &e_cnt}) v->resize(c0 + n);
        layers.resize(l0 + nl);
        for (auto* v : {&meta, &w_lo, &w_hi}) v->resize(e0 + ne);
        sigma.resize((e0 + ne) * sigma_words);
        pvac_ct_batch X{};
        X.n = n;
        X.l_off = l_off.data() + c0; X.l_cnt = l_cnt.data() + c0; X.e_off = e_off.data() + c0; X.e_cnt = e_cnt.data() + c0;
        X.layers = layers.data() + l0;
        X.meta = meta.data() + e0; X.w_lo = w_lo.data() + e0; X.w_hi = w_hi.data() + e0;
        X.sigma = sigma_words ? sigma.data() + e0 * sigma_words : nullptr;
        X.sigma_words = sigma_words;
        MUST(pvac_ct_parse(file.data(), file.size(), &X, 1) == PVAC_OK, "parse");
        for (size_t i = c0; i < c0 + n; ++i) {   // offsets into the pool's arrays
            l_off[i] += l0;
            e_off[i] += e0;
        }
    }

    // the file image of ciphers ids[0], ids[1], ... of the pool
    std::vector<uint8_t> image(const std::vector<size_t>& ids) {
        std::vector<uint64_t> lo, lc, eo, ec;
        for (size_t i : ids) {
            lo.push_back(l_off[i]); lc.push_back(l_cnt[i]); eo.push_back(e_off[i]); ec.push_back(e_cnt[i]);
        }
        pvac_ct_batch X{};
        X.n = ids.size();
        X.l_off = lo.data(); X.l_cnt = lc.data(); X.e_off = eo.data(); X.e_cnt = ec.data();
        X.layers = layers.data();
        X.meta = meta.data(); X.w_lo = w_lo.data(); X.w_hi = w_hi.data();
        X.sigma = sigma_words ? sigma.data() : nullptr;
        X.sigma_words = sigma_words;
        uint64_t bytes = 0, written = 0;
        MUST(pvac_ct_serialized_size(&X, sigma_bits, &bytes) == PVAC_OK, "size");
        std::vector<uint8_t> out(bytes);
        MUST(pvac_ct_write(&X, sigma_bits, out.data(), out.size(), &written, 1) == PVAC_OK && written == bytes, "write");
        return out;
    }
};

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <file.ct> ... | --mismatch <a.ct> <b.ct>\n", argv[0]);
        return 2;
    }
    pvac_hip_params prm{};
    prm.B = 337;
    prm.m_bits = 8192;
    prm.n_bits = 16384;
    prm.h_col_wt = 192;
    prm.x_col_wt = 128;
    prm.err_wt = 128;
    prm.edge_budget = 1200000;
    pvac_hip::Engine eng(0, prm);
    if (!std::strcmp(argv[1], "--mismatch")) {
        MUST(argc == 4, "--mismatch takes two files");
        const pvac_hip::device_batch A = eng.batch_from_image(slurp(argv[2])), B = eng.batch_from_image(slurp(argv[3]));
        MUST(A.sigma_bits != B.sigma_bits, "the two files agree on sigma nbits");
        bool threw = false;
        try {
            (void)eng.concat({&A, &B});
        } catch (const pvac_hip::Error& e) {
            threw = e.code == PVAC_EINVAL;
        }
        MUST(threw, "sources that disagree on sigma_bits were concatenated");
        std::printf("%d checks passed\n", g_checks);
        return 0;
    }
    host_pool pool;
    std::vector<pvac_hip::device_batch> dev;
    for (int a = 1; a < argc; ++a) {
        const std::vector<uint8_t> file = slurp(argv[a]);
        pool.add(file);
        dev.push_back(eng.batch_from_image(file));
        MUST(dev.back().sigma_bits == pool.sigma_bits, "%s: sigma_bits", argv[a]);
    }
    pool.first.push_back(pool.l_cnt.size());
    std::vector<const pvac_hip::device_batch*> srcs;
    for (const pvac_hip::device_batch& d : dev) srcs.push_back(&d);
    const size_t nf = dev.size(), total = pool.l_cnt.size();

    // concat: all ciphers in file order
    std::vector<size_t> all(total);
    for (size_t i = 0; i < total; ++i) all[i] = i;
    pvac_hip::device_batch cat = eng.concat(srcs);
    MUST(cat.sigma_bits == pool.sigma_bits && cat.view().n == total, "concat: %llu ciphers", (unsigned long long)cat.view().n);
    MUST(eng.ct_image(cat.view(), cat.sigma_bits) == pool.image(all), "concat: the image differs from the host regrouping");

    // gather: files in reverse order, each one's ciphers reversed, its last cipher twice; with several
    // files the middle ones' are left out
    std::vector<uint32_t> ps;
    std::vector<uint64_t> pi;
    std::vector<size_t> ids;
    for (size_t f = nf; f-- > 0;) {
        if (nf > 2 && f != 0 && f != nf - 1) continue;
        const size_t n = pool.first[f + 1] - pool.first[f];
        for (size_t c = n; c-- > 0;) {
            for (int rep = 0; rep < (c == n - 1 ? 2 : 1); ++rep) {
                ps.push_back((uint32_t)f);
                pi.push_back(c);
                ids.push_back(pool.first[f] + c);
            }
        }
    }
    pvac_hip::device_batch got = eng.gather(srcs, ps, pi);
    MUST(got.view().n == ids.size(), "gather: %llu ciphers", (unsigned long long)got.view().n);
    MUST(eng.ct_image(got.view(), got.sigma_bits) == pool.image(ids), "gather: the image differs from the host regrouping");

    // one source, pick_src left out; no picks at all is the empty batch
    std::vector<uint64_t> rev;
    for (size_t c = pool.first[1]; c-- > 0;) rev.push_back(c);
    pvac_hip::device_batch one = eng.gather({srcs[0]}, {}, rev);
    MUST(eng.ct_image(one.view(), one.sigma_bits) == pool.image(std::vector<size_t>(rev.begin(), rev.end())), "gather from one source");
    pvac_hip::device_batch none = eng.gather(srcs, {}, {});
    MUST(none.view().n == 0 && eng.ct_image(none.view(), none.sigma_bits) == pool.image({}), "the empty gather");

    // a pick beyond its source is refused
    bool threw = false;
    try {
        (void)eng.gather(srcs, {0}, {(uint64_t)pool.first[1]});
    } catch (const pvac_hip::Error& e) {
        threw = e.code == PVAC_EINVAL;
    }
    MUST(threw, "a pick beyond its source was accepted");
    std::printf("%d checks passed\n", g_checks);
    return 0;
}
