// commit_binding_check.cpp — compile/link check of the INTEGRATION.md §2 binding of commit_ct against
// the REAL reference headers (pvac-hfhe 0.1.0): the function below is the body a maintainer puts under
// PVAC_USE_MI355X in ops/commit.hpp, instantiated on pvac::PubKey / Cipher (core/types.hpp:72-139).
// Built and linked by tests/test_commit_binding.py only where the reference exists; never run, never
// shipped.
#include <pvac/pvac.hpp>
#include <pvac_hip.hpp>

#include <array>
#include <type_traits>

namespace binding {

using pvac::Cipher;
using pvac::PubKey;

std::array<uint8_t, 32> commit_ct(const PubKey& pk, const Cipher& C) { return pvac_hip::commit_ct(pk, C); }   // commit.hpp:12
std::vector<std::array<uint8_t, 32>> commit_ct_batch(const PubKey& pk, const std::vector<Cipher>& cs) {
    return pvac_hip::commit_ct_batch(pk, cs);
}

static_assert(std::is_same<decltype(pvac_hip::commit_ct(std::declval<const PubKey&>(), std::declval<const Cipher&>())),
                           decltype(pvac::commit_ct(std::declval<const PubKey&>(), std::declval<const Cipher&>()))>::value,
              "commit_ct returns what the reference's returns");

}  // namespace binding

int main(int argc, char**) {
    // link check only: reference every binding so nothing is discarded
    volatile void* keep[] = {(void*)&binding::commit_ct, (void*)&binding::commit_ct_batch};
    return argc > 99 ? (int)(uintptr_t)keep[0] : 0;
}
