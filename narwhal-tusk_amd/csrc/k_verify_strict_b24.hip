// k_verify_strict_b24.hip -- verify kernels, strict mode, 24-bit comb of B (one translation
// unit per mode and comb width, so the build compiles them in parallel).
#include "k_verify.inc"

namespace nt {
template hipError_t launch_verify_m<kStrict, kBCombBits>(uint64_t, const uint8_t*, const uint8_t*, const uint8_t*, uint64_t,
                                              const uint64_t*, const uint64_t*, uint64_t, const uint32_t*, void*,
                                              uint64_t*, hipStream_t, int, XTab, KTabArgs);
}  // namespace nt
