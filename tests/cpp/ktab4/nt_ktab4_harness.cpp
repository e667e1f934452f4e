// nt_ktab4_harness.cpp -- TEST INFRASTRUCTURE: the four-table path of the verify kernel's
// key-table cache on the host (ktab_tables.hpp ktab_build with an extension, ladder_k4,
// verify_k4; ed25519_ops.hpp compare_one) over memory the test owns.  Never linked into libntcrypto.so.
#include "k4_common.hpp"

namespace {
// one verification through verify_n<MODE, 1> with a cache that has an extension (or a null one)
int verify_kt4(int mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint64_t len, const HostKTab4& kt) {
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

static_assert(kKtHasExt<HostKTab4> && !kKtHasExt<HostKTab> && !kKtHasExt<NoKTab>, "the extension trait defaults to off");

extern "C" {
int ntk4_ext_bytes() { return (int)kKtExtBytes; }

// ktab_build (four tables) + verify_k4; mode 0 strict, 1 cofactorless
int ntk4_verify(int mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint64_t len) {
  return k4::verify(mode, pk, sig, msg, len);
}

// out32 = the encoding of ladder_k4's [k](-A) over the key's four tables; returns the
// entry's header flags, or a negative build error.  dead = 1: the lane is told its key has no tables.
int ntk4_ladder(const uint8_t* pk, const uint8_t* k32, int dead, uint8_t* out32) {
  alignas(16) uint32_t A[8], k[8];
  words(A, pk);
  words(k, k32);
  k4::OneKey key;
  if (const int e = key.build(A)) return e;
  ge_cp t;
  ladder_k4(t, k, dead ? 1u : 0u, key.kt(), 0u);
  ge_p2 P;
  ge_cp_to_p2(P, t);
  uint32_t w[8];
  ge_tobytes_w(w, P);
  std::memcpy(out32, w, 32);
  return (int)key.flags;
}

// the 64 signed digits ladder_k4 takes of k (sc_recode_w4), as int8
void ntk4_digits(const uint8_t* k32, int8_t* out64) {
  uint32_t k[8], d[8];
  words(k, k32);
  sc_recode_w4(d, k);
  for (int i = 0; i < 64; ++i) out64[i] = (int8_t)w4_digit(d, i);
}

// compare_one<MODE> of R' = (x z : y z : z) with the encoding R32 (x, y, z: 32-byte field
// elements, z != 0), the strict small-order test as verify_k4 asks for it
int ntk4_compare(int mode, const uint8_t* x32, const uint8_t* y32, const uint8_t* z32, const uint8_t* R32) {
  uint32_t xw[8], yw[8], zw[8], Rw[8];
  words(xw, x32);
  words(yw, y32);
  words(zw, z32);
  words(Rw, R32);
  fe x, y, z, zi;
  fe_frombytes_w(x, xw);
  fe_frombytes_w(y, yw);
  fe_frombytes_w(z, zw);
  ge_p2 P;
  fe_mul(P.X, x, z);
  fe_mul(P.Y, y, z);
  P.Z = z;
  fe_invert_batch(zi, z);
  return (int)(mode == 0 ? compare_one<kStrict>(P, zi, Rw, true) : compare_one<kCofactorless>(P, zi, Rw, false));
}

// The bytes ktab_build writes for one key: kind 0 = the three-table policy (HostKTab), 1 = a
// policy with a null extension, 2 = with an extension.  pool: kKtEntryBytes, ext: kKtExtBytes,
// both prefilled by the caller.  Returns 0, or a negative error.
int ntk4_build(const uint8_t* pk, int kind, uint8_t* pool, uint8_t* ext) {
  alignas(16) uint32_t A[8];
  words(A, pk);
  uint64_t slots[kKtBucket] = {};
  uint32_t ctl[4] = {};
  if (kind == 0) {
    const HostKTab kt{slots, kKtBucket - 1, pool, 1, ctl};
    ktab_build(A, 3u, kt);
  } else {
    const HostKTab4 kt(slots, kKtBucket - 1, pool, 1, ctl, kind == 2 ? ext : nullptr);
    ktab_build(A, 3u, kt);
  }
  return slots[3] == ktab_word(ktab_fp(A), kKtReady0) && ctl[0] == 1 ? 0 : -1;
}

// n verifications, one after the other, through the whole path (verify_n) with the cache the
// caller owns, as ntk_verify_many of the three-table harness; ext: cap entries of
// ntk4_ext_bytes(), or nullptr for a cache without a fourth table.
void ntk4_verify_many(int mode, uint64_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                      const uint64_t* off, const uint64_t* len, uint64_t* slots, uint32_t smask, uint8_t* pool,
                      uint32_t cap, uint8_t* ext, uint32_t* ctl, uint8_t* out) {
  const HostKTab4 kt(slots, smask, pool, cap, ctl, ext);
  for (uint64_t i = 0; i < n; ++i) out[i] = (uint8_t)verify_kt4(mode, pk + 32 * i, sig + 64 * i, msg + off[i], len[i], kt);
}
}
