// nt_xcache_harness.cpp -- TEST INFRASTRUCTURE: the x cache of the verify kernel
// (ed25519_ops.hpp XCache, ge_frombytes_cached) on the host, over a plain array
// the test fills with whatever it likes.  Built on the host harness
// (../nt_host_harness.cpp: its HostATab, its comb of B and its operation
// counters), which is included as source so that nothing of it is restated.
// Never linked into libntcrypto.so.
#include "../nt_host_harness.cpp"

namespace {
// `msk + 1` slots of 8 words, indexed like the device table
struct HostXCache {
  static constexpr bool kEnabled = true;
  uint32_t* tab;
  uint32_t msk;
  int* stores;
  bool active() const { return tab != nullptr; }
  uint32_t mask() const { return msk; }
  void load(uint32_t i, uint32_t xw[8]) const { std::memcpy(xw, tab + 8 * (size_t)(i & msk), 32); }
  void store(uint32_t i, const uint32_t xw[8]) const {
    std::memcpy(tab + 8 * (size_t)(i & msk), xw, 32);
    ++*stores;
  }
};
}  // namespace

extern "C" {
// the 8 candidate slots of a key in a table of mask + 1 slots
void nthx_slots(const uint8_t* pk, uint32_t mask, uint32_t* out8) {
  uint32_t A[8];
  words(A, pk);
  const uint32_t b0 = xcache_bucket(xcache_hash(A, 0x9e3779b9u), mask);
  const uint32_t b1 = xcache_bucket(xcache_hash(A, 0x7f4a7c15u), mask);
  for (uint32_t c = 0; c < kXCand; ++c) out8[c] = xcache_cand(b0, b1, c, mask);
}

// Decompression of one key through the cache: returns bit 0 = decodes, bit 1 = the
// square root was skipped (counted: the slow path squares 250 times and more, the
// check once), bit 2 = the slot was written; x32 / t32 = canonical X and T = X Y of
// the point handed on.  tab == nullptr: no table.
int nthx_frombytes(const uint8_t* pk, uint32_t* tab, uint32_t mask, uint8_t* x32, uint8_t* t32) {
  uint32_t A[8], w[8];
  words(A, pk);
  int stores = 0;
  const HostXCache xc{tab, mask, &stores};
  ge_p3 P;
  const unsigned long long s0 = g_fe_sq;
  const uint32_t ok = ge_frombytes_cached(P, A, xc);
  const bool skipped = g_fe_sq - s0 < 2 + kXCand;
  fe_tobytes_w(w, P.X);
  std::memcpy(x32, w, 32);
  fe_tobytes_w(w, P.T);
  std::memcpy(t32, w, 32);
  return (int)ok | (skipped ? 2 : 0) | (stores ? 4 : 0);
}

// One verification (mode 0 strict, 1 cofactorless) with the key's x served from the
// table: the verdict, as nth_verify gives it without a table.
int nthx_verify(int mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint64_t len, uint32_t* tab,
                uint32_t mask) {
  alignas(16) uint32_t A[8], S[16];
  std::memcpy(A, pk, 32);
  std::memcpy(S, sig, 64);
  const uint32_t* Ap[1] = {A};
  const uint32_t* Sp[1] = {S};
  const uint8_t* Mp[1] = {msg};
  const uint64_t Lp[1] = {len};
  uint32_t ok[1];
  HostATab at;
  int stores = 0;
  const HostXCache xc{tab, mask, &stores};
  if (mode == 0) verify_n<kStrict, 1>(ok, Ap, Sp, Mp, Lp, at, bcomb(), xc);
  else verify_n<kCofactorless, 1>(ok, Ap, Sp, Mp, Lp, at, bcomb(), xc);
  return (int)ok[0];
}
}
