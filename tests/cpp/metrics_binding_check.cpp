// metrics_binding_check.cpp — compile/link check of the INTEGRATION.md §2 binding of the metrics
// (utils/metrics.hpp) against the REAL reference headers (pvac-hfhe 0.1.0): each function below is the
// body a maintainer puts under PVAC_USE_MI355X in utils/metrics.hpp, instantiated on pvac::PubKey /
// Cipher / Fp (core/types.hpp:72-139, core/field.hpp). Built and linked by
// tests/test_metrics_binding.py only where the reference exists; never run, never shipped.
#include <pvac/pvac.hpp>
#include <pvac_hip.hpp>

#include <type_traits>

namespace binding {

using pvac::Cipher;
using pvac::Fp;
using pvac::PubKey;

// metrics.hpp:43 has no PubKey parameter; the routed form takes the key the caller's workload holds
double sigma_shannon(const PubKey& pk, const Cipher& C) { return pvac_hip::sigma_shannon(pk, C); }
std::vector<double> sigma_shannon_batch(const PubKey& pk, const std::vector<Cipher>& cs) {
    return pvac_hip::sigma_shannon_batch(pk, cs);
}
Fp agg_layer_gsum(const PubKey& pk, const Cipher& X, uint32_t lid) { return pvac_hip::agg_layer_gsum<Fp>(pk, X, lid); }   // metrics.hpp:70
std::vector<std::vector<Fp>> layer_gsums_batch(const PubKey& pk, const std::vector<Cipher>& cs) {
    return pvac_hip::layer_gsums_batch<Fp>(pk, cs);
}
void dump_metrics(const PubKey& pk, const char* tag, const Cipher& C, const Fp& val) {                                    // metrics.hpp:13
    pvac_hip::dump_metrics(pk, tag, C, val);
}

static_assert(std::is_same<decltype(pvac_hip::agg_layer_gsum<Fp>(std::declval<const PubKey&>(), std::declval<const Cipher&>(),
                                                                 0u)),
                           Fp>::value,
              "agg_layer_gsum returns the reference's Fp");
static_assert(std::is_same<decltype(pvac_hip::sigma_shannon(std::declval<const PubKey&>(), std::declval<const Cipher&>())),
                           decltype(pvac::sigma_shannon(std::declval<const Cipher&>()))>::value,
              "sigma_shannon returns what the reference's returns");

}  // namespace binding

int main(int argc, char**) {
    // link check only: reference every binding so nothing is discarded
    volatile void* keep[] = {(void*)&binding::sigma_shannon, (void*)&binding::sigma_shannon_batch,
                             (void*)&binding::agg_layer_gsum, (void*)&binding::layer_gsums_batch,
                             (void*)&binding::dump_metrics};
    return argc > 99 ? (int)(uintptr_t)keep[0] : 0;
}
