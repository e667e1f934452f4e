// k4_common.hpp -- TEST INFRASTRUCTURE: one key's four tables built by ktab_build into a
// private one-entry pool + extension, and verify_k4 over them.  Shared by the ctypes harness
// (nt_ktab4_harness.cpp) and the stand-alone sanitizer program (k4_corpus_main.cpp).  Built on
// the host harness (../nt_host_harness.cpp: its comb of B), which is included as source so that
// nothing of it is restated.
#pragma once
#include "../nt_host_harness.cpp"
#include "host_ktab4.hpp"

namespace k4 {
// a one-entry cache of its own: 8 index slots, one pool entry, one extension entry
struct OneKey {
  uint64_t slots[kKtBucket] = {};
  alignas(16) uint8_t pool[kKtEntryBytes] = {};
  alignas(16) uint8_t ext[kKtExtBytes] = {};
  uint32_t ctl[4] = {};
  uint32_t flags = 0;
  HostKTab4 kt(bool with_ext = true) { return HostKTab4(slots, kKtBucket - 1, pool, 1, ctl, with_ext ? ext : nullptr); }
  // the claimer of slot 3 builds entry 0; 0 = published with the key's tag
  int build(const uint32_t A[8], bool with_ext = true) {
    const HostKTab4 t = kt(with_ext);
    ktab_build(A, 3u, t);
    if (slots[3] != ktab_word(ktab_fp(A), kKtReady0)) return -1;
    uint32_t tag[8];
    t.hdr_load(0, tag, flags);
    return std::memcmp(tag, A, 32) != 0 ? -2 : 0;
  }
};

// build + verify_k4 of one signature: the verdict, or a negative build error
inline int verify(int mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint64_t len) {
  alignas(16) uint32_t A[8], S[16];
  std::memcpy(A, pk, 32);
  std::memcpy(S, sig, 64);
  OneKey key;
  if (const int e = key.build(A)) return e;
  uint32_t k[8];
  hram_scalar(k, S, A, msg, len);
  const HostKTab4 kt = key.kt();
  return (int)(mode == 0 ? verify_k4<kStrict>(S, S + 8, k, key.flags, bcomb(), kt, 0u)
                         : verify_k4<kCofactorless>(S, S + 8, k, key.flags, bcomb(), kt, 0u));
}
}  // namespace k4
