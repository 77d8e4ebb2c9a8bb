// deep_ops.hpp — what ct_lincomb, compact and ct_recrypt accept of a deep cipher, and the route a
// ct_lincomb term takes. Plain host / device arithmetic with no HIP in it: the plan kernels, the host
// runtime and tests/cpp/deep_ops_check.cpp (a stand-alone host program) all read it from here.
//
// 30,000 is what k_ct_add's LDS keep table holds (120 KB). Up to there every table sized by a layer count
// lives in LDS; a context whose layer limit was raised above it (pvac_hip_ctx_set_layer_limit) admits
// more, and such a cipher takes code whose tables are in global scratch. At the default limit the bound
// is 30,000 and nothing below moves.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PVAC_DEEP_HD __host__ __device__
#else
#define PVAC_DEEP_HD
#endif

namespace pvhip {

constexpr uint32_t kLinWaveLayers = 64;
constexpr uint32_t kLinWaveEdges = 8192;
constexpr uint32_t kLinMaxLayers = 30000;   // per term on the workgroup route: its LDS keep table (and k_ct_add's)

// the most layers a ct_lincomb term or fold-route segment, a cipher of compact's merge set and a ct_recrypt
// sum may have on a context with this layer limit: ct_add's own rule
PVAC_DEEP_HD inline uint32_t deep_layer_bound(uint32_t layer_limit) {
    return layer_limit > kLinMaxLayers ? layer_limit : kLinMaxLayers;
}

// ct_lincomb, per term: who finds the layers compact_layers keeps
//   wave   a lane group, the keep set a 64-bit mask
//   wg     one workgroup, keep table in LDS, the remap left in the slab
//   deep   one workgroup, keep table and remap both in the slab
// The slab (lincomb_args::remap) holds one word per input layer slot of the call; term k's words start
// at sL[k], the exclusive scan of the terms' layer counts that also gives C.l_off. So the slab is sized
// by that scan's total, and no two terms share a word however often a cipher is a term.
enum : uint32_t { LIN_ROUTE_WAVE = 0, LIN_ROUTE_WG = 1, LIN_ROUTE_DEEP = 2 };
PVAC_DEEP_HD inline uint32_t lincomb_route(uint64_t L, uint64_t E) {
    if (L <= kLinWaveLayers && E <= kLinWaveEdges) return LIN_ROUTE_WAVE;
    return L <= kLinMaxLayers ? LIN_ROUTE_WG : LIN_ROUTE_DEEP;
}

}  // namespace pvhip
