// deep_ops_binding_check.cpp — compile/link check of the adapter's deep-cipher flow (include/pvac_hip.hpp)
// next to the REAL reference headers (pvac-hfhe 0.1.0): the reference's loop c = ct_mul(pk, c, x) grows a
// cipher past 30,000 layers at step 13 and recrypts it (ops/recrypt.hpp:26-41); here the caller raises the
// engine's layer limit once and the same calls pass the cipher through, with deep_route_counts() beside the
// limit to see which route served it. Built and linked by tests/test_deep_ops_binding.py only where the
// reference exists; never run, never shipped.
#include <pvac/pvac.hpp>
#include <pvac_hip.hpp>

#include <array>
#include <type_traits>

namespace binding {

using pvac::Cipher;
using pvac::EvalKey;
using pvac::PubKey;

// the limit of the calling thread's engine for this key; the free functions below then take deep ciphers
void allow_deep(const PubKey& pk, uint32_t layers) { pvac_hip::engine_for(pk).set_layer_limit(layers); }

Cipher sum_of_chain_outputs(const PubKey& pk, const std::vector<Cipher>& cs) { return pvac_hip::ct_sum(pk, cs, true); }
std::vector<Cipher> inner_products(const PubKey& pk, const std::vector<Cipher>& X, const std::vector<uint64_t>& seg_off,
                                   const std::vector<uint64_t>& term, const std::vector<pvac::Fp>& scales) {
    return pvac_hip::ct_lincomb_batch(pk, X, seg_off, term, scales, {}, true);
}
void compact_edges(const PubKey& pk, Cipher& C) { pvac_hip::compact_edges(pk, C); }
Cipher ct_recrypt(const PubKey& pk, const EvalKey& ek, const Cipher& in) { return pvac_hip::ct_recrypt(pk, ek, in); }
std::array<uint64_t, 4> routes(const PubKey& pk) { return pvac_hip::engine_for(pk).deep_route_counts(); }

static_assert(std::is_same<decltype(std::declval<const pvac_hip::Engine&>().deep_route_counts()), std::array<uint64_t, 4>>::value,
              "four counters, as pvac_hip_deep_route_count fills them");
static_assert(std::is_same<decltype(&pvac_hip_deep_route_count), int (*)(pvac_hip_ctx*, uint64_t*)>::value,
              "the ABI entry point's prototype");

}  // namespace binding

int main(int argc, char**) {
    // link check only: reference every binding so nothing is discarded
    volatile void* keep[] = {(void*)&binding::allow_deep,    (void*)&binding::sum_of_chain_outputs, (void*)&binding::inner_products,
                             (void*)&binding::compact_edges, (void*)&binding::ct_recrypt,           (void*)&binding::routes};
    return argc > 99 ? (int)(uintptr_t)keep[0] : 0;
}
