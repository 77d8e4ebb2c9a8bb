// lincomb_flatten_check.cpp — the adapter's host arithmetic for ct_lincomb without a GPU:
// pvac_hip::detail::flatten_lincomb (include/pvac_hip.hpp) checks a call's ragged lists against the pool
// and turns Fp scales into the C ABI's words. Stand-alone (tests/test_lincomb_binding.py builds it with
// -fsanitize=address,undefined and runs it).
#include <cstdio>
#include <vector>

#include "pvac_hip.hpp"

struct Fp { uint64_t lo, hi; };
using U = std::vector<uint64_t>;
using F = std::vector<uint32_t>;

static int g_fail = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::fprintf(stderr, "FAIL %d: %s\n", __LINE__, #c);    \
            ++g_fail;                                               \
        }                                                           \
    } while (0)

static bool refused(size_t n_x, const U& seg_off, const U& term, const std::vector<Fp>& scales, const F& flags) {
    try {
        (void)pvac_hip::detail::flatten_lincomb(n_x, seg_off, term, scales, flags);
    } catch (const pvac_hip::Error& e) {
        return e.code == PVAC_EINVAL;
    }
    return false;
}

int main() {
    using pvac_hip::detail::flatten_lincomb;
    const std::vector<Fp> none;
    {   // ragged segments with empty ones, repeated terms, scales over the whole word range
        const U seg_off{0, 0, 3, 3, 4}, term{2, 0, 2, 1};
        const std::vector<Fp> sc{{0, 0}, {1, 0}, {~0ull, ~0ull >> 1}, {~0ull, ~0ull}};
        const auto s = flatten_lincomb(3, seg_off, term, sc, F{1, 0, 1, 1});
        CHECK(s.seg_off == seg_off && s.term == term);
        CHECK((s.scale == U{0, 0, 1, 0, ~0ull, ~0ull >> 1, ~0ull, ~0ull}));
        CHECK((s.flags == F{1, 0, 1, 1}));
        const auto t = flatten_lincomb(3, seg_off, term, sc, F{});   // every term scaled
        CHECK(t.flags.empty() && t.scale.size() == 8);
        const auto u = flatten_lincomb(3, seg_off, term, none, F{});   // nothing scaled
        CHECK(u.scale.empty() && u.flags.empty());
    }
    {   // no outputs, and outputs without terms
        const auto s = flatten_lincomb(0, U{}, U{}, none, F{});
        CHECK(s.seg_off == U{0} && s.term.empty());
        const auto t = flatten_lincomb(0, U{0, 0, 0}, U{}, none, F{});
        CHECK(t.seg_off.size() == 3);
    }
    CHECK(refused(3, U{1, 2}, U{0, 1}, none, F{}));            // does not start at 0
    CHECK(refused(3, U{0, 1}, U{0, 1}, none, F{}));            // does not end at the number of terms
    CHECK(refused(3, U{0, 2, 1, 2}, U{0, 1}, none, F{}));      // decreases
    CHECK(refused(3, U{0, 2}, U{0, 3}, none, F{}));            // a term index = |X|
    CHECK(refused(0, U{0, 1}, U{0}, none, F{}));               // any term of an empty pool
    CHECK(refused(3, U{0, 2}, U{0, 1}, {{1, 0}}, F{}));        // one scale for two terms
    CHECK(refused(3, U{0, 2}, U{0, 1}, {{1, 0}, {2, 0}}, F{1}));   // one flag for two terms
    CHECK(refused(3, U{0, 2}, U{0, 1}, none, F{1, 1}));        // flags without scales
    CHECK(refused(3, U{}, U{0}, none, F{}));                   // terms without an output
    if (g_fail) return 1;
    std::printf("lincomb_flatten_check: ok\n");
    return 0;
}
