// nt_kcomb_harness.cpp -- TEST INFRASTRUCTURE: the comb path of the verify kernel's key-table
// cache on the host (ed25519_ops.hpp ktab_build with a comb pool; ktab_comb.hpp kc_recode / kc_pick,
// ladder_kc, verify_kc) over memory the test owns.  Never linked into libntcrypto.so.
#include "kc_common.hpp"

namespace {
// one verification through verify_n<MODE, 1> with a cache whose second pool holds combs (or is null)
int verify_ktc(int mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint64_t len, const HostKComb& kt) {
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

static_assert(kKtHasComb<HostKComb> && !kKtHasExt<HostKComb> && !kKtHasComb<HostKTab> && !kKtHasComb<NoKTab>,
              "the comb trait defaults to off");

extern "C" {
int ntkc_comb_bytes() { return (int)kKtCombBytes; }

// ktab_build (comb) + verify_kc; mode 0 strict, 1 cofactorless
int ntkc_verify(int mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint64_t len) {
  return kc::verify(mode, pk, sig, msg, len);
}

// out32 = the encoding of ladder_kc's [k](-A) over the key's comb; returns the entry's header
// flags, or a negative build error.  dead = 1: the lane is told its key has no comb.
int ntkc_ladder(const uint8_t* pk, const uint8_t* k32, int dead, uint8_t* out32) {
  alignas(16) uint32_t A[8], k[8];
  words(A, pk);
  words(k, k32);
  kc::OneKey key;
  if (const int e = key.build(A)) return e;
  ge_cp t;
  ladder_kc(t, k, dead ? 1u : 0u, key.kt(), 0u);
  ge_p2 P;
  ge_cp_to_p2(P, t);
  uint32_t w[8];
  ge_tobytes_w(w, P);
  std::memcpy(out32, w, 32);
  return (int)key.flags;
}

// the 64 lookups ladder_kc takes of k, in its order (columns 15 .. 0, blocks 0 .. 3 within a
// column): out[3 i] = block, out[3 i + 1] = index within the block, out[3 i + 2] = negate;
// returns c (1: the correction adds +A)
int ntkc_recode(const uint8_t* k32, int32_t* out192) {
  uint32_t k[8];
  words(k, k32);
  uint64_t slots[kKtBucket] = {};
  uint32_t ctl[4] = {};
  const HostKComb kt(slots, kKtBucket - 1, nullptr, 0, ctl, nullptr);
  kc_recode(k, kt);
  int i = 0;
  for (uint32_t col = kKcCols; col-- > 0;)
    for (uint32_t j = 0; j < kKcBlocks; ++j, ++i) {
      const uint32_t pk = kc_pick(kt, col, j);
      out192[3 * i] = (int32_t)((pk & 0xffu) / kKcPerBlock);
      out192[3 * i + 1] = (int32_t)((pk & 0xffu) % kKcPerBlock);
      out192[3 * i + 2] = (int32_t)(pk >> 8);
    }
  return (int)kt.dig_get(8u);
}

// The bytes ktab_build writes for one key, as entry `idx` of `cap`: kind 0 = the three-table policy
// (HostKTab), 1 = a comb policy with a null comb pool, 2 = with a comb pool.  pool: cap x
// kKtEntryBytes, comb: cap x kKtCombBytes, both prefilled by the caller.  Returns 0, or a negative error.
int ntkc_build(const uint8_t* pk, int kind, uint8_t* pool, uint8_t* comb, uint32_t cap, uint32_t idx) {
  alignas(16) uint32_t A[8];
  words(A, pk);
  uint64_t slots[kKtBucket] = {};
  uint32_t ctl[4] = {idx, 0, 0, 0};
  HostATab at;
  if (kind == 0) {
    const HostKTab kt{slots, kKtBucket - 1, pool, cap, ctl};
    ktab_build(A, 3u, kt, at);
  } else {
    const HostKComb kt(slots, kKtBucket - 1, pool, cap, ctl, kind == 2 ? comb : nullptr);
    ktab_build(A, 3u, kt, at);
  }
  return slots[3] == ktab_word(ktab_fp(A), kKtReady0 + idx) && ctl[0] == idx + 1 ? 0 : -1;
}

// n verifications, one after the other, through the whole path (verify_n) with the cache the
// caller owns; comb: cap entries of ntkc_comb_bytes(), or nullptr for a cache without combs.
void ntkc_verify_many(int mode, uint64_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                      const uint64_t* off, const uint64_t* len, uint64_t* slots, uint32_t smask, uint8_t* pool,
                      uint32_t cap, uint8_t* comb, uint32_t* ctl, uint8_t* out) {
  const HostKComb kt(slots, smask, pool, cap, ctl, comb);
  for (uint64_t i = 0; i < n; ++i) out[i] = (uint8_t)verify_ktc(mode, pk + 32 * i, sig + 64 * i, msg + off[i], len[i], kt);
}
}
