// deep_ops_check.cpp — csrc/deep_ops.hpp without a GPU: the layer bound that ct_lincomb, compact and
// ct_recrypt take from a context's layer limit, the route of a ct_lincomb term at 30,000 / 30,001 / the
// limit / the limit + 1, the slab of keep / remap words (offsets by the scan of the terms' layer counts,
// grown through dev_buf against the fake allocator of fake_hip.hpp), and the classification at the default
// limit against the rule the runtime had before the deep-term route, restated here in numbers. Host code
// only, no libamdhip64; built with ASan + UBSan by deep_ops.mk (tests/test_deep_ops_host.py).
#include "fake_hip.hpp"

#include <algorithm>

#include "deep_ops.hpp"
#include "dev_mem.hpp"
#include "pvac_hip.h"

using namespace pvhip;

namespace {

// what a plan does with a term of L layers and E edges: 0 wave, 1 workgroup, 2 deep-term route, -1 refused
int plan_term(uint64_t L, uint64_t E, uint32_t limit) {
    if (L > deep_layer_bound(limit)) return -1;
    return (int)lincomb_route(L, E);
}

// the rule before the deep-term route existed, whatever the limit
int plan_term_before(uint64_t L, uint64_t E) {
    if (L > 30000) return -1;
    return (L <= 64 && E <= 8192) ? 0 : 1;
}

void check_bound() {
    CHECK(PVAC_LAYER_LIMIT_DEFAULT == 16384u && kLinMaxLayers == 30000u, "the constants the rule is stated in");
    CHECK(deep_layer_bound(PVAC_LAYER_LIMIT_DEFAULT) == 30000u, "the default limit leaves the bound at 30000");
    CHECK(deep_layer_bound(29999) == 30000u && deep_layer_bound(30000) == 30000u, "a limit below 30000 does not lower it");
    CHECK(deep_layer_bound(30001) == 30001u && deep_layer_bound(1u << 17) == (1u << 17), "above, the bound is the limit");
    CHECK(deep_layer_bound(PVAC_LAYER_LIMIT_MAX) == PVAC_LAYER_LIMIT_MAX, "up to the largest limit");
}

void check_routes() {
    const uint32_t limit = 1u << 17;
    CHECK(plan_term(30000, 40, limit) == LIN_ROUTE_WG, "30000 layers: the workgroup route, its table in LDS");
    CHECK(plan_term(30001, 40, limit) == LIN_ROUTE_DEEP, "30001 layers: the deep-term route");
    CHECK(plan_term(limit, 40, limit) == LIN_ROUTE_DEEP, "the limit itself is accepted");
    CHECK(plan_term((uint64_t)limit + 1, 40, limit) == -1, "one layer above the limit is refused");
    CHECK(plan_term(30001, 0, limit) == LIN_ROUTE_DEEP && plan_term(30001, 1ull << 30, limit) == LIN_ROUTE_DEEP,
          "the edge count does not move a deep term");
    CHECK(plan_term(64, 8192, limit) == LIN_ROUTE_WAVE && plan_term(65, 0, limit) == LIN_ROUTE_WG &&
              plan_term(64, 8193, limit) == LIN_ROUTE_WG && plan_term(0, 0, limit) == LIN_ROUTE_WAVE,
          "the wave route's edge of 64 layers and 8192 edges stays");
    // a raised limit changes nothing at or below 30000 layers
    for (uint64_t L : {0ull, 1ull, 64ull, 65ull, 1024ull, 16384ull, 29999ull, 30000ull})
        for (uint64_t E : {0ull, 1ull, 8192ull, 8193ull, 1ull << 20})
            for (uint32_t lim : {PVAC_LAYER_LIMIT_DEFAULT, 30001u, limit, PVAC_LAYER_LIMIT_MAX})
                CHECK(plan_term(L, E, lim) == plan_term_before(L, E), "L = %llu, E = %llu at limit %u",
                      (unsigned long long)L, (unsigned long long)E, lim);
}

void check_default_limit() {
    // at the default limit (and at any limit up to 30000) every shape is planned as before
    const uint64_t Ls[] = {0, 1, 2, 32, 63, 64, 65, 100, 1023, 1024, 1025, 8212, 16384, 16385, 29999, 30000,
                           30001, 30002, 32792, 65536, 1u << 17, (1u << 24) + 1, 1ull << 31, 1ull << 40};
    const uint64_t Es[] = {0, 1, 39, 8191, 8192, 8193, 65536, 1200000, 1ull << 31};
    for (uint32_t lim : {PVAC_LAYER_LIMIT_DEFAULT, 20000u, 30000u})
        for (uint64_t L : Ls)
            for (uint64_t E : Es) {
                const int now = plan_term(L, E, lim);
                CHECK(now == plan_term_before(L, E) && now != (int)LIN_ROUTE_DEEP, "L = %llu, E = %llu at limit %u",
                      (unsigned long long)L, (unsigned long long)E, lim);
            }
}

// The slab: one word per input layer slot of the call, term k's words at the exclusive scan of the layer
// counts. A cipher that is a term twice has two regions.
void check_slab() {
    const uint64_t layers[] = {3, 30001, 70, 30001, 0, 131072, 64, 30000, 32792, 32792, 8212};
    const size_t n = sizeof layers / sizeof layers[0];
    uint64_t off[n + 1];
    uint64_t run = 0;
    for (size_t k = 0; k < n; ++k) {
        off[k] = run;
        run += layers[k];
    }
    off[n] = run;
    CHECK(run == 3 + 30001 + 70 + 30001 + 131072 + 64 + 30000 + 32792 + 32792 + 8212, "the scan's total");
    const size_t at = g_log.size();
    dev_buf<uint32_t> slab;
    CHECK(slab.grow_floor(run) == hipSuccess && slab.capacity() >= run, "the slab holds the scan's total");
    EXPECT_CALLS(at, ("M" + std::to_string(4 * run)).c_str());
    size_t deep = 0;
    for (size_t k = 0; k < n; ++k) {
        if (lincomb_route(layers[k], 10) != LIN_ROUTE_DEEP) continue;
        ++deep;
        CHECK(off[k] + layers[k] == off[k + 1] && off[k + 1] <= slab.capacity(), "term %zu inside the slab", k);
        for (size_t j = 0; j < n; ++j)   // no word shared with another term's region
            CHECK(j == k || off[j] + layers[j] <= off[k] || off[k] + layers[k] <= off[j], "terms %zu and %zu overlap", k, j);
        uint32_t* keep = slab.get() + off[k];   // the first and last word a deep term's workgroup touches
        keep[0] = 1;
        keep[layers[k] - 1] = 1;
    }
    CHECK(deep == 5, "five deep terms in the table");
    // a second, smaller call keeps the buffer
    const uint32_t* held = slab.get();
    CHECK(slab.grow_floor(30001) == hipSuccess && slab.get() == held, "no regrowth below capacity");
}

}  // namespace

int main() {
    check_bound();
    check_routes();
    check_default_limit();
    check_slab();
    CHECK(g_live.size() == 0, "every block was freed");
    if (g_fail) {
        std::printf("deep_ops_check: %d FAILED\n", g_fail);
        return 1;
    }
    std::printf("deep_ops_check: ok\n");
    return 0;
}
