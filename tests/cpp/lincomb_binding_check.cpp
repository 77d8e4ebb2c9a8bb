// lincomb_binding_check.cpp — compile/link check of the INTEGRATION.md binding of ct_sum / ct_lincomb /
// ct_lincomb_batch against the REAL reference headers (pvac-hfhe 0.1.0): each function below is what a
// maintainer adds to ops/arithmetic.hpp under PVAC_USE_MI355X, instantiated on pvac::PubKey / Cipher /
// Fp (core/types.hpp:72-139, core/field.hpp:17-20). Built and linked by tests/test_lincomb_binding.py
// only where the reference exists; never run, never shipped.
#include <pvac/pvac.hpp>
#include <pvac_hip.hpp>

#include <type_traits>

namespace binding {

using pvac::Cipher;
using pvac::Fp;
using pvac::PubKey;

Cipher ct_sum(const PubKey& pk, const std::vector<Cipher>& cs) { return pvac_hip::ct_sum(pk, cs); }
Cipher ct_lincomb(const PubKey& pk, const std::vector<Cipher>& cs, const std::vector<Fp>& scales) {
    return pvac_hip::ct_lincomb(pk, cs, scales);
}
std::vector<Cipher> ct_lincomb_batch(const PubKey& pk, const std::vector<Cipher>& X, const std::vector<uint64_t>& seg_off,
                                     const std::vector<uint64_t>& term, const std::vector<Fp>& scales,
                                     const std::vector<uint32_t>& flags) {
    return pvac_hip::ct_lincomb_batch(pk, X, seg_off, term, scales, flags);
}

static_assert(std::is_same<decltype(pvac_hip::ct_sum(std::declval<const PubKey&>(), std::declval<const std::vector<Cipher>&>())),
                           Cipher>::value,
              "ct_sum returns the reference's Cipher");
static_assert(std::is_same<decltype(pvac_hip::detail::flatten_lincomb(size_t(0), std::declval<const std::vector<uint64_t>&>(),
                                                                      std::declval<const std::vector<uint64_t>&>(),
                                                                      std::declval<const std::vector<Fp>&>(),
                                                                      std::declval<const std::vector<uint32_t>&>())),
                           pvac_hip::detail::lincomb_lists>::value,
              "the reference's Fp flattens into scale words");

}  // namespace binding

int main(int argc, char**) {
    // link check only: reference every binding so nothing is discarded
    volatile void* keep[] = {(void*)&binding::ct_sum, (void*)&binding::ct_lincomb, (void*)&binding::ct_lincomb_batch};
    return argc > 99 ? (int)(uintptr_t)keep[0] : 0;
}
