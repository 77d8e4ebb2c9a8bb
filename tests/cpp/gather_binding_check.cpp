// gather_binding_check.cpp — compile/link check of the adapter's regrouping calls (Engine::gather /
// Engine::concat, include/pvac_hip.hpp) next to the REAL reference headers (pvac-hfhe 0.1.0): the flow a
// maintainer writes where the reference would load two ciphertext files, push their Ciphers into one
// std::vector and save it (tests/add.cpp: loadCts / saveCts), here without the ciphers leaving the
// device. Built and linked by tests/test_gather_binding.py only where the reference exists; never run,
// never shipped.
#include <pvac/pvac.hpp>
#include <pvac_hip.hpp>

#include <type_traits>

namespace binding {

using pvac::PubKey;

// two .ct files become one in a single step
std::vector<uint8_t> merge_ct_files(const PubKey& pk, const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
    pvac_hip::Engine eng(0, pvac_hip::Engine::params_of(pk));
    const pvac_hip::device_batch A = eng.batch_from_image(a), B = eng.batch_from_image(b);
    pvac_hip::device_batch all = eng.concat({&A, &B});
    return eng.ct_image(all.view(), all.sigma_bits);
}

// keep some ciphers of several resident batches, in any order
pvac_hip::device_batch pick(pvac_hip::Engine& eng, const std::vector<const pvac_hip::device_batch*>& srcs,
                            const std::vector<uint32_t>& which_batch, const std::vector<uint64_t>& which_cipher) {
    return eng.gather(srcs, which_batch, which_cipher);
}

static_assert(std::is_same<decltype(std::declval<pvac_hip::Engine&>().concat(std::declval<const std::vector<const pvac_hip::device_batch*>&>())),
                           pvac_hip::device_batch>::value,
              "concat returns a batch that owns its arrays");
static_assert(std::is_same<decltype(std::declval<pvac_hip::Engine&>().gather(std::declval<const std::vector<const pvac_hip::device_batch*>&>(),
                                                                             std::declval<const std::vector<uint32_t>&>(),
                                                                             std::declval<const std::vector<uint64_t>&>())),
                           pvac_hip::device_batch>::value,
              "gather returns a batch that owns its arrays");
static_assert(PVAC_GATHER_MAX_SOURCES == 1024, "the source limit of the ABI");

}  // namespace binding

int main(int argc, char**) {
    // link check only: reference every binding so nothing is discarded
    volatile void* keep[] = {(void*)&binding::merge_ct_files, (void*)&binding::pick};
    return argc > 99 ? (int)(uintptr_t)keep[0] : 0;
}
