// recrypt_binding_check.cpp — compile/link check of the INTEGRATION.md §2 binding of ct_recrypt and its
// parts against the REAL reference headers (pvac-hfhe 0.1.0): each function below is the body a
// maintainer puts under PVAC_USE_MI355X in ops/recrypt.hpp, ops/encrypt.hpp and crypto/matrix.hpp,
// instantiated on pvac::PubKey / SecKey / EvalKey / Cipher (core/types.hpp:72-139). Built and linked
// by tests/test_recrypt_binding.py only where the reference exists; never run, never shipped.
#include <pvac/pvac.hpp>
#include <pvac_hip.hpp>

#include <type_traits>

namespace binding {

using pvac::Cipher;
using pvac::EvalKey;
using pvac::PubKey;
using pvac::SecKey;

double sigma_density(const PubKey& pk, const Cipher& C) { return pvac_hip::sigma_density(pk, C); }         // encrypt.hpp:29
void ubk_apply(const PubKey& pk, Cipher& C) { pvac_hip::ubk_apply(pk, C); }                               // matrix.hpp:306
void compact_edges(const PubKey& pk, Cipher& C) { pvac_hip::compact_edges(pk, C); }                       // encrypt.hpp:39
Cipher ct_recrypt(const PubKey& pk, const EvalKey& ek, const Cipher& in) { return pvac_hip::ct_recrypt(pk, ek, in); }   // recrypt.hpp:26
std::vector<Cipher> ct_recrypt_batch(const PubKey& pk, const EvalKey& ek, const std::vector<Cipher>& in) {
    return pvac_hip::ct_recrypt_batch(pk, ek, in);
}
EvalKey make_evalkey(const PubKey& pk, const SecKey& sk, size_t pool_size, int depth_hint) {             // recrypt.hpp:12
    return pvac_hip::make_evalkey<EvalKey>(pk, sk, pool_size, depth_hint);
}

static_assert(std::is_same<decltype(pvac_hip::ct_recrypt(std::declval<const PubKey&>(), std::declval<const EvalKey&>(),
                                                         std::declval<const Cipher&>())),
                           Cipher>::value,
              "ct_recrypt returns the reference's Cipher");
static_assert(pvac_hip::detail::has_ubk<PubKey>::value, "engine_for uploads pk.ubk.inv of the reference's PubKey");

}  // namespace binding

int main(int argc, char**) {
    // link check only: reference every binding so nothing is discarded
    volatile void* keep[] = {(void*)&binding::sigma_density, (void*)&binding::ubk_apply,        (void*)&binding::compact_edges,
                             (void*)&binding::ct_recrypt,    (void*)&binding::ct_recrypt_batch, (void*)&binding::make_evalkey};
    return argc > 99 ? (int)(uintptr_t)keep[0] : 0;
}
