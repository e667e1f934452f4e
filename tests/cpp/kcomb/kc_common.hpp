// kc_common.hpp -- TEST INFRASTRUCTURE: one key's comb built by ktab_build into a private
// one-entry pool + comb pool, and verify_kc over it.  Shared by the ctypes harness
// (nt_kcomb_harness.cpp) and the stand-alone sanitizer program (kcomb_main.cpp).  Built on the
// host harness (../nt_host_harness.cpp: its comb of B and table workspace), which is included as
// source so that nothing of it is restated.
#pragma once
#include "../nt_host_harness.cpp"
#include "host_kcomb.hpp"

namespace kc {
// a one-entry cache of its own: 8 index slots, one pool entry, one comb
struct OneKey {
  uint64_t slots[kKtBucket] = {};
  alignas(16) uint8_t pool[kKtEntryBytes] = {};
  alignas(16) uint8_t comb[kKtCombBytes] = {};
  uint32_t ctl[4] = {};
  uint32_t flags = 0;
  HostKComb kt() { return HostKComb(slots, kKtBucket - 1, pool, 1, ctl, comb); }
  // the claimer of slot 3 builds entry 0; 0 = published with the key's tag
  int build(const uint32_t A[8]) {
    const HostKComb t = kt();
    HostATab at;
    ktab_build(A, 3u, t, at);
    if (slots[3] != ktab_word(ktab_fp(A), kKtReady0)) return -1;
    uint32_t tag[8];
    t.hdr_load(0, tag, flags);
    return std::memcmp(tag, A, 32) != 0 ? -2 : 0;
  }
};

// build + verify_kc of one signature: the verdict, or a negative build error
inline int verify(int mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint64_t len) {
  alignas(16) uint32_t A[8], S[16];
  std::memcpy(A, pk, 32);
  std::memcpy(S, sig, 64);
  OneKey key;
  if (const int e = key.build(A)) return e;
  uint32_t k[8];
  hram_scalar(k, S, A, msg, len);
  const HostKComb kt = key.kt();
  return (int)(mode == 0 ? verify_kc<kStrict>(S, S + 8, k, key.flags, bcomb(), kt, 0u)
                         : verify_kc<kCofactorless>(S, S + 8, k, key.flags, bcomb(), kt, 0u));
}
}  // namespace kc
