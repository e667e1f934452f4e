// nt_ktab_harness.cpp -- TEST INFRASTRUCTURE: the unbalanced lattice vector
// (sc25519.hpp sc_unbalanced), the three-table ladder (ktab_tables.hpp
// verify_uv3) and the key-table cache (KTab) on the host, over memory the test
// owns and may fill with whatever it likes.  Built on the host harness
// (../nt_host_harness.cpp: its HostATab and its comb of B), which is included as
// source so that nothing of it is restated.  Never linked into libntcrypto.so.
#include "../nt_host_harness.cpp"
#include "host_ktab.hpp"

namespace {
// one verification through verify_n<MODE, 1> with the cache
int verify_kt(int mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint64_t len, const HostKTab& kt) {
  alignas(16) uint32_t A[8], S[16];
  std::memcpy(A, pk, 32);
  std::memcpy(S, sig, 64);
  const uint32_t* Ap[1] = {A};
  const uint32_t* Sp[1] = {S};
  const uint8_t* Mp[1] = {msg};
  const uint64_t Lp[1] = {len};
  uint32_t ok[1];
  HostATab at;
  if (mode == 0) verify_n<kStrict, 1>(ok, Ap, Sp, Mp, Lp, at, bcomb(), NoXCache(), kt);
  else verify_n<kCofactorless, 1>(ok, Ap, Sp, Mp, Lp, at, bcomb(), NoXCache(), kt);
  return (int)ok[0];
}
}  // namespace

extern "C" {
int ntk_entry_bytes() { return (int)kKtEntryBytes; }
int ntk_candidates() { return (int)kKtCand; }

// sc_unbalanced_t<lehmer> of n scalars (8 words each): u, v (8 words), sign of u, bit lengths
void ntk_unbalanced(uint64_t n, const uint32_t* k8, uint32_t* u8, uint32_t* uneg, uint32_t* v8, int32_t* ubits,
                    int32_t* vbits, int lehmer) {
  for (uint64_t i = 0; i < n; ++i) {
    int ub, vb;
    if (lehmer) sc_unbalanced_t<true>(u8 + 8 * i, uneg[i], v8 + 8 * i, k8 + 8 * i, ub, vb);
    else sc_unbalanced_t<false>(u8 + 8 * i, uneg[i], v8 + 8 * i, k8 + 8 * i, ub, vb);
    ubits[i] = ub;
    vbits[i] = vb;
  }
}

// The ntk_candidates() candidate slots of a key in an index of smask + 1 slots, and its fingerprint.
uint32_t ntk_slots(const uint8_t* pk, uint32_t smask, uint32_t* out32) {
  uint32_t A[8];
  words(A, pk);
  const uint32_t bm = smask / kKtBucket;
  const uint32_t b0 = (xcache_hash(A, 0x51ed270bu) & bm) * kKtBucket;
  const uint32_t b1 = (xcache_hash(A, 0x2545f491u) & bm) * kKtBucket;
  for (uint32_t c = 0; c < kKtCand; ++c) out32[c] = ((c < kKtBucket ? b0 : b1) | (c & (kKtBucket - 1))) & smask;
  return xcache_hash(A, 0x94d049bbu);
}

// verify_uv3 with the key's tables built by ktab_build into a private one-entry
// pool, for the lattice vector `which`: 0 unbalanced, 1 balanced (sc_halfsize),
// 2 trivial (k, 1).  mode 0 strict, 1 cofactorless.
int ntk_verify_uv3(int mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint64_t len, int which) {
  alignas(16) uint32_t A[8], S[16];
  std::memcpy(A, pk, 32);
  std::memcpy(S, sig, 64);
  uint64_t slots[kKtBucket] = {};
  alignas(16) static thread_local uint8_t pool[kKtEntryBytes];
  std::memset(pool, 0, sizeof pool);
  uint32_t ctl[4] = {};
  const HostKTab kt{slots, kKtBucket - 1, pool, 1, ctl};
  ktab_build(A, 3u, kt);
  if (slots[3] != ktab_word(ktab_fp(A), kKtReady0)) return -1;
  uint32_t tag[8], flags;
  kt.hdr_load(0, tag, flags);
  if (std::memcmp(tag, A, 32) != 0) return -2;
  uint32_t k[8], u[8], v[8] = {1, 0, 0, 0, 0, 0, 0, 0}, uneg = 0;
  int ub = 253, vb = 1;
  hram_scalar(k, S, A, msg, len);
  if (which == 0) {
    sc_unbalanced(u, uneg, v, k, ub, vb);
  } else if (which == 1) {
    ub = vb = sc_halfsize(u, uneg, v, k);
  } else {
    std::memcpy(u, k, 32);
  }
  HostATab at;
  return (int)(mode == 0 ? verify_uv3<kStrict>(S, S + 8, u, uneg, v, ub, vb, flags, at, bcomb(), kt, 0u)
                         : verify_uv3<kCofactorless>(S, S + 8, u, uneg, v, ub, vb, flags, at, bcomb(), kt, 0u));
}

// n verifications, one after the other ("one thread"), through the whole path with
// the cache the caller owns: slots (smask + 1 words of 8 bytes), pool (cap entries
// of ntk_entry_bytes()), ctl (4 words: entries handed out, fast rows, builds,
// old-path rows).  slots == nullptr: no cache.  out[i] = verdict.
void ntk_verify_many(int mode, uint64_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                     const uint64_t* off, const uint64_t* len, uint64_t* slots, uint32_t smask, uint8_t* pool,
                     uint32_t cap, uint32_t* ctl, uint8_t* out) {
  const HostKTab kt{slots, smask, pool, cap, ctl};
  for (uint64_t i = 0; i < n; ++i) out[i] = (uint8_t)verify_kt(mode, pk + 32 * i, sig + 64 * i, msg + off[i], len[i], kt);
}
}
