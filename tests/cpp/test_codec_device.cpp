// test_codec_device.cpp — the device .ct codec through the C++ adapter (include/pvac_hip.hpp). Runs on
// the GPU box:
//   test_codec_device <file.ct> ...
// every file goes through Engine::batch_from_image (host index, one upload, device parse) and
// Engine::ct_image (device image, one download) and must come back as the same bytes; the parsed
// counts must be the file's. Exit 0 = every check passed; failures abort with a message.
#include <cstdio>
#include <cstdlib>
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

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <file.ct> ...\n", argv[0]);
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
    for (int a = 1; a < argc; ++a) {
        const std::vector<uint8_t> file = slurp(argv[a]);
        pvac_ct_file_info info{};
        MUST(pvac_ct_scan(file.data(), file.size(), &info) == PVAC_OK, "%s: scan", argv[a]);
        pvac_hip::device_batch X = eng.batch_from_image(file);
        MUST(X.sigma_bits == info.sigma_bits, "%s: sigma_bits %u", argv[a], X.sigma_bits);
        const pvac_ct_batch v = X.view();
        MUST(v.n == info.n_ciphers, "%s: %llu ciphers", argv[a], (unsigned long long)v.n);
        MUST((v.sigma != nullptr) == (info.sigma_words != 0), "%s: sigma rows", argv[a]);
        const std::vector<uint8_t> back = eng.ct_image(v, info.sigma_bits);
        MUST(back == file, "%s: the image of the parsed batch differs from the file (%zu / %zu bytes)", argv[a], back.size(), file.size());
    }
    // not a file: refused on the host, before anything is uploaded
    bool threw = false;
    try {
        (void)eng.batch_from_image(std::vector<uint8_t>(40, 0));
    } catch (const pvac_hip::Error& e) {
        threw = e.code == PVAC_EINVAL;
    }
    MUST(threw, "a zero block was accepted as a .ct file");
    std::printf("%d checks passed\n", g_checks);
    return 0;
}
