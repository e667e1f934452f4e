// ktab_tables.hpp -- the key-table cache's window-table generations, superseded
// by the comb (ktab_comb.hpp) and kept as A/B builds (-DNT_KCOMB=0, -DNT_KTAB4=0)
// and for the host harnesses and the device probe: the three-table path
// (ktab_build, ladder_a3r, ladder_uv3, verify_uv3) and the four-table path
// (KtStore's extension arm, ladder_k4, verify_k4).  Nothing the comb path calls
// is here.  A part of ed25519_ops.hpp, included after ktab.hpp: include that
// file, not this one.
//
// Three tables: the window tables j * P, j = 1..8, of P = A, A' = [2^64]A and
// A'' = [2^128]A.  With them the lattice vector need not be balanced:
// |u| ~ 2^192, v ~ 2^64 (sc_unbalanced), the 4-bit digits of |u| split into three
// strings of 16 over the three tables, and the joint ladder is ~17 windows of
// 4 doublings + 4 additions instead of ~33 of 4 + 2 (verify_uv3).  [u]A =
// [u0]A + [u1]A' + [u2]A'' is an integer identity (A', A'' come from real
// doublings of A), so the verdict is verify_uv's for every input.
// Four tables: with A''' = [2^192]A in the extension pool (ktab.hpp) the whole k
// splits into four strings of 16 digits, and the cached verify needs no lattice
// vector and nothing of R but its bytes (verify_k4).
#pragma once

namespace nt {

// ATab-shaped store adaptor of ptab_build: entries 1..8 of table t of pool entry idx
// (t = kKtTables: the extension's table)
template <class KT>
struct KtStore {
  const KT& kt;
  uint32_t idx, t, on;
  NT_HD NT_INLINE void store(uint32_t entry, const ge_cached& c) {
    if (!on || entry == 0) return;
    if constexpr (kKtHasExt<KT>) {
      if (t >= kKtTables) {
        kt.ext_store(idx, entry, c);
        return;
      }
    }
    kt.tab_store(idx, t, entry, c);
  }
};

// Build and publish the entries of the lanes with claim != kKtNoSlot (their keys' index slots).  Wave-uniform:
// every lane of the row runs the arithmetic (on its own key), only the claimers
// store.  128 doublings and three ptab_builds in a rolled loop, once per key; with an
// extension pool one round more (192 doublings, four ptab_builds), the fourth table
// stored like the others before the drain: all of an entry's lines, then drain, release,
// drain, then the slot word.  Without one (a null extension address, or a three-table
// policy) exactly the three tables are built and nothing else is stored.
// Undecodable keys get the header alone, with the flag (the full tag makes a
// negative entry safe); small-order keys get the flag beside their tables.
template <class KT>
NT_HD NT_INLINE void ktab_build(const uint32_t Aw[8], uint32_t claim, const KT& kt) {
  const uint32_t fp = ktab_fp(Aw);
  uint32_t idx = 0, have = 0;
  if (claim != kKtNoSlot) {
    idx = kt.pool_take();
    have = idx < kt.capacity() ? 1u : 0u;
    if (!have) kt.slot_store(claim, ktab_word(fp, kKtSeen));  // pool exhausted: seen for good
  }
  ge_p3 P;
  const uint32_t ok = ge_frombytes_w(P, Aw);
  const uint32_t flags = (ok ? 0u : kKtUndecodable) | (ge_is_small_order_affine(P) ? kKtSmallOrder : 0u);
  KtStore<KT> st{kt, idx, 0, have & ok};
  const uint32_t ntab = kKtTables + (ktab_has_ext(kt) ? 1u : 0u);
#pragma unroll 1
  for (uint32_t t = 0; t < ntab; ++t) {
    st.t = t;
    ptab_build(P, 0u, st, 0);
    if (t + 1 < ntab) {
      ge_p2 q;
      ge_p3_to_p2(q, P);
#pragma unroll 1
      for (int r = 0; r < 63; ++r) ge_dbl_p2(q, q);
      ge_cp c;
      ge_dbl(c, q);
      ge_cp_to_p3(P, c);
    }
  }
  if (have) kt.hdr_store(idx, Aw, flags);
  // every storing wave drains and releases before any slot word names its entry
  kt.drain_release();
  if (have) kt.slot_publish(claim, ktab_word(fp, kKtReady0 + idx));
}

// t = -[u]A - [v]R (completed) from the key's three cached tables (pool entry
// kidx; dead: the lane has no tables, its A digits are taken as zero) and the
// lane's own table of -R: W windows, 4 (W - 1) doublings.  Window wi adds R's digit
// wi and, of |u|'s 64 digits, digit wi of the first 16 on A, digit 16 + wi on A',
// digit 32 + wi of the last 32 on A'' -- so any W <= 64 is right for any valid
// vector, (k, 1) included.  The sign of u is folded into the digit.
// The 16 digit words (v's at 0..7, |u|'s at 8..15) wait with kt.dig_put / dig_get (the kernel:
// LDS) and a window reads the four it needs: held in registers through this loop they are the
// first thing the allocator spills, and it then reloads them from scratch window by window.
template <class KT>
NT_HD NT_INLINE int32_t kt_digit(const KT& kt, uint32_t word0, int wi) {
  return (int32_t)(((kt.dig_get(word0 + (uint32_t)(wi >> 3)) >> (4 * (wi & 7))) & 15u) ^ 8u) - 8;
}
template <class ATab, class KT>
NT_HD NT_INLINE void ladder_a3r(ge_cp& t, uint32_t uneg, int W, const ATab& at, const KT& kt, uint32_t kidx) {
#pragma unroll 1
  for (int wi = W - 1; wi >= 0; --wi) {
    int j = 0;
    if (wi == W - 1) {
      ge_cached ce;
      at.load_signed(kTabR, kt_digit(kt, 0, wi), ce);
      // cached -> completed with T = Z (as ladder_ar's seed)
      fe_sub4(t.X, ce.YpX, ce.YmX);
      fe_carry(t.X);
      fe_add(t.Y, ce.YpX, ce.YmX);
      fe_carry(t.Y);
      t.Z = ce.Z2;
      t.T = ce.Z2;
      j = 1;
    } else {
      ge_p2 acc;
      ge_cp_to_p2(acc, t);
#pragma unroll 1
      for (int r = 0; r < 3; ++r) ge_dbl_p2(acc, acc);
      ge_dbl(t, acc);
    }
    // additions 0: R, 1: A'' (wi < 32), 2: A', 3: A (wi < 16).  The window's four digits are
    // taken here and packed, so that the rolled loop below indexes nothing.
    const int nj = wi < 16 ? 4 : (wi < 32 ? 2 : 1);
    const int wl = wi & 15;
    const uint32_t dpack = ((uint32_t)kt_digit(kt, 0, wi) & 15u) | (((uint32_t)kt_digit(kt, 12, wi & 31) & 15u) << 4) |
                           (((uint32_t)kt_digit(kt, 10, wl) & 15u) << 8) | (((uint32_t)kt_digit(kt, 8, wl) & 15u) << 12);
#pragma unroll 1
    for (; j < nj; ++j) {
      const int32_t d = (int32_t)(((dpack >> (4 * j)) & 15u) ^ 8u) - 8;  // sign-extended nibble
      ge_cached ce;
      if (j == 0) {
        at.load_signed(kTabR, d, ce);
      } else {
        kt.tab_load_signed(kidx, 3u - (uint32_t)j, uneg ? d : -d, ce);  // -[u]A = [|u|](u < 0 ? A : -A)
      }
      ge_p3 q;
      ge_cp_to_p3(q, t);
      ge_add_cached(t, q, ce);
    }
  }
}

// verify_uv3's variable-base part, t = -[u]A - [v]R (completed): the digits of |u| and v
// parked for ladder_a3r (dead: the key has no tables, its digits are zero), the window count
// of the vector's bit lengths -- every lane of a wave runs its wave's largest -- and the ladder.
// at holds the lane's table of -R already.
template <class ATab, class KT>
NT_HD NT_INLINE void ladder_uv3(ge_cp& t, const uint32_t u[8], uint32_t uneg, const uint32_t v[8], int ubits,
                                int vbits, uint32_t dead, const ATab& at, const KT& kt, uint32_t kidx) {
  uint32_t ud[8], vd[8];
  sc_recode_w4(ud, u);
  sc_recode_w4(vd, v);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    kt.dig_put((uint32_t)i, vd[i]);
    kt.dig_put(8u + (uint32_t)i, dead ? 0u : ud[i]);
  }
  // 4 windows(b) >= b + 2: the signed top digit absorbs the carry
  const int wv = (vbits + 5) >> 2, wu = ((ubits + 5) >> 2) - 32;
  int Wn = wv > wu ? wv : wu;
  Wn = Wn < 16 ? 16 : (Wn > 64 ? 64 : Wn);
  const int W = wave_max(Wn);
  ladder_a3r(t, uneg, W, at, kt, kidx);
}

// verify_uv for a key whose tables are cached: (u, v) any valid vector of k with
// bit lengths <= ubits, vbits (verify_one uses sc_unbalanced's; the tests also run
// the balanced one and (k, 1)); kflags = the entry's header flags.
template <int MODE, class ATab, class WComb, class KT>
NT_HD NT_INLINE uint32_t verify_uv3(const uint32_t Rw[8], const uint32_t Sw[8], const uint32_t u[8], uint32_t uneg,
                                    const uint32_t v[8], int ubits, int vbits, uint32_t kflags, ATab& at,
                                    const WComb& wb, const KT& kt, uint32_t kidx) {
  const uint32_t dead = (kflags & kKtUndecodable) ? 1u : 0u;
  uint32_t ok = sc_is_canonical(Sw) & (dead ^ 1u);
  if (MODE == kStrict) ok &= (kflags & kKtSmallOrder) ? 0u : 1u;
  {
    ge_p3 R;
    ok &= ge_frombytes_w(R, Rw);
    if (MODE == kStrict) ok &= ge_is_small_order_affine(R) ^ 1u;
    ptab_build(R, 1u, at, kTabR);
  }
  uint32_t w[8];
  sc_mul(w, v, Sw);
  ge_cp t;
  ladder_uv3(t, u, uneg, v, ubits, vbits, dead, at, kt, kidx);
  ge_p3 acc;
  ge_cp_to_p3(acc, t);
  wcomb_acc(acc, w, wb);
  return ok & fe_iszero(acc.X) & fe_eq(acc.Y, acc.Z);
}

// t = [k](-A) (completed) for the full k < L from the key's FOUR cached tables (pool
// entry kidx and its extension; dead: the key has no tables, its digits are taken as
// zero): exactly 16 windows, 60 doublings, 64 additions, nothing of R and no lattice
// vector.  k is recoded once into 64 signed nibbles; k < L < 2^253, so the top nibble is
// at most 1 + carry and absorbs the carry (sc_recode_w4's bound, 2^255 - 2^251, is far
// away).  Window wi adds digit wi on A, 16 + wi on A', 32 + wi on A'', 48 + wi on A''',
// each with its sign flipped (the tables hold +A).  The 8 digit words wait with
// kt.dig_put / dig_get as ladder_a3r's do.  The first window seeds the accumulator from
// its first addition and doubles nothing.
template <class KT>
NT_HD NT_INLINE void ladder_k4(ge_cp& t, const uint32_t k[8], uint32_t dead, const KT& kt, uint32_t kidx) {
  {
    uint32_t kd[8];
    sc_recode_w4(kd, k);
#pragma unroll
    for (int i = 0; i < 8; ++i) kt.dig_put((uint32_t)i, dead ? 0u : kd[i]);
  }
#pragma unroll 1
  for (int wi = 15; wi >= 0; --wi) {
    // string s has its 16 digits in words 2s, 2s + 1: the window's four, packed, so that the
    // rolled loop below indexes nothing
    const uint32_t dpack = ((uint32_t)kt_digit(kt, 0, wi) & 15u) | (((uint32_t)kt_digit(kt, 2, wi) & 15u) << 4) |
                           (((uint32_t)kt_digit(kt, 4, wi) & 15u) << 8) | (((uint32_t)kt_digit(kt, 6, wi) & 15u) << 12);
    if (wi != 15) {
      ge_p2 acc;
      ge_cp_to_p2(acc, t);
#pragma unroll 1
      for (int r = 0; r < 3; ++r) ge_dbl_p2(acc, acc);
      ge_dbl(t, acc);
    }
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const int32_t d = 8 - (int32_t)(((dpack >> (4 * j)) & 15u) ^ 8u);  // the nibble, sign-extended and negated
      ge_cached ce;
      if (j == 3) kt.ext_load_signed(kidx, d, ce);
      else kt.tab_load_signed(kidx, (uint32_t)j, d, ce);
      if (wi == 15 && j == 0) {
        // cached -> completed with T = Z (as ladder_ar's seed)
        fe_sub4(t.X, ce.YpX, ce.YmX);
        fe_carry(t.X);
        fe_add(t.Y, ce.YpX, ce.YmX);
        fe_carry(t.Y);
        t.Z = ce.Z2;
        t.T = ce.Z2;
      } else {
        ge_p3 q;
        ge_cp_to_p3(q, t);
        ge_add_cached(t, q, ce);
      }
    }
  }
}

// The check for a key whose four tables are cached (kflags = the entry's header flags),
// k = the full hash scalar:
//   ok  <=>  s < L, A decodes, (strict) A is not of small order, and R' = [s]B - [k]A
//            encodes to R's bytes the way dalek compares points (enc_matches), (strict)
//            R' not of small order
// -- verify_uv's verdict for every input: with v odd and below L, [v]([s]B - [k]A - R) is
// the identity only if R decodes to R' itself.  R is never decompressed, the lane's table
// workspace is not touched, and s goes to the comb as it is.
template <int MODE, class WComb, class KT>
NT_HD NT_INLINE uint32_t verify_k4(const uint32_t Rw[8], const uint32_t Sw[8], const uint32_t k[8], uint32_t kflags,
                                   const WComb& wb, const KT& kt, uint32_t kidx) {
  const uint32_t dead = (kflags & kKtUndecodable) ? 1u : 0u;
  uint32_t ok = sc_is_canonical(Sw) & (dead ^ 1u);
  if (MODE == kStrict) ok &= (kflags & kKtSmallOrder) ? 0u : 1u;
  ge_cp t;
  ladder_k4(t, k, dead, kt, kidx);
  ge_p3 acc;
  ge_cp_to_p3(acc, t);
  wcomb_acc(acc, Sw, wb);
  fe zi;
  fe_invert_batch(zi, acc.Z);
  ge_p2 P;
  ge_p3_to_p2(P, acc);
  return ok & compare_one<MODE>(P, zi, Rw, MODE == kStrict);
}

}  // namespace nt
