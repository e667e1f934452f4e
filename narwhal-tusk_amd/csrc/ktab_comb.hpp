// ktab_comb.hpp -- the key-table cache's comb, what the product runs on a cached
// row: the build of a key's 33 comb lines (ktab_build_comb), the recoding of the
// hash scalar, the ladder and the verdict (kc_recode, ladder_kc, verify_kc).  A
// part of ed25519_ops.hpp, included after ktab.hpp: include that file, not this
// one.
#pragma once

namespace nt {

// The comb.  The second pool holds, per entry index, a Lim-Lee comb of A with
// kKcTeeth = 4 teeth 64 bits apart and kKcBlocks = 4 blocks of kKcCols = 16 columns: 33 affine
// niels entries (y+x, y-x, 2dxy), one 128-B line each (120 B used), kKtCombBytes per key.
//   entry 8 j + e   2^(16 j) (2^192 + r2 2^128 + r1 2^64 + r0) A,  r_t = +1 if bit t of e is set, else -1
//   entry 32        A itself
// With K = k | 1 and W = (K >> 1) | 2^255, the signs s_i = 2 bit_i(W) - 1 give
// sum s_i 2^i = 2 W - (2^256 - 1) = K as an INTEGER, so [K]A is the sum of 64 signed entries
// for every A, torsion component or not: column `col` of block j takes bits 16 j + col of the
// four 64-bit limbs of W, the top tooth's sign factored out (ladder_kc: 15 doublings, 64
// mixed additions, and one more of entry 32 or the identity for the parity of k).  A policy
// says that it can carry one with `static constexpr bool kComb = true` and then has
//   has_comb() (wave-uniform: the second pool is there and holds combs),
//   comb_store(idx, entry, niels), comb_load(idx, entry, niels&)
// Only the entry's 128-B header is written beside a comb: no window table is built.
constexpr uint32_t kKcTeeth = 4, kKcBlocks = 4, kKcCols = 16, kKcPerBlock = 1u << (kKcTeeth - 1);
constexpr uint32_t kKcSigned = kKcBlocks * kKcPerBlock;  // 32 signed entries, then +A
constexpr uint32_t kKcEntries = kKcSigned + 1, kKcLineBytes = 128;
constexpr uint32_t kKtCombBytes = kKcEntries * kKcLineBytes;  // 4,224
static_assert(kKcTeeth * kKcBlocks * kKcCols == 256 && kKcBlocks * kKcCols == 64,
              "a tooth is one 64-bit limb of W; the recoding below is written for four of them");

// The comb's build parks its 16 bases in entries 0 .. 15 of the lane's table workspace.  Every
// ATab that verify_uv takes holds the two window tables of the balanced path, entries
// 0 .. kTabR + 8; a policy that states its size (`static constexpr uint32_t kEntries`) is checked
// against the 16 as well.
constexpr uint32_t kKcBases = kKcTeeth * kKcBlocks;
static_assert(kKcBases <= kTabR + 9, "the comb's bases wait in the balanced path's table workspace");
template <class ATab>
constexpr auto atab_entries_of(int) -> decltype(ATab::kEntries) { return ATab::kEntries; }
template <class ATab>
constexpr uint32_t atab_entries_of(long) { return kTabR + 9; }
// four field elements parked in one entry of the lane's table workspace (ATab::store / load
// move a ge_cached as it is): a p3 point, or a cached one
template <class ATab>
NT_HD NT_INLINE void kc_park_p3(ATab& at, uint32_t entry, const ge_p3& p) {
  const ge_cached c{p.X, p.Y, p.Z, p.T};
  at.store(entry, c);
}
template <class ATab>
NT_HD NT_INLINE void kc_take_p3(const ATab& at, uint32_t entry, ge_p3& p) {
  ge_cached c;
  at.load(entry, c);
  p.X = c.YpX; p.Y = c.YmX; p.Z = c.Z2; p.T = c.T2d;
}
// comb line `entry` of pool entry idx for a lane that stores (on), nothing and zeros otherwise
template <class KT>
NT_HD NT_INLINE void kc_line_put(const KT& kt, uint32_t idx, uint32_t entry, const ge_niels& q, uint32_t on) {
  if (on) kt.comb_store(idx, entry, q);
}
template <class KT>
NT_HD NT_INLINE void kc_line_get(const KT& kt, uint32_t idx, uint32_t entry, ge_niels& q, uint32_t on) {
  fe_0(q.ypx); fe_0(q.ymx); fe_0(q.xy2d);
  if (on) kt.comb_load(idx, entry, q);
}
// p + q and p - q (completed -> p3)
NT_HD NT_INLINE void kc_add_sub(ge_p3& sum, ge_p3& dif, const ge_p3& p, const ge_p3& q) {
  ge_cached c;
  ge_p3_to_cached(c, q);
  ge_cp t;
  ge_add_cached(t, p, c);
  ge_cp_to_p3(sum, t);
  ge_cached_cneg(c, 1u);
  ge_add_cached(t, p, c);
  ge_cp_to_p3(dif, t);
}

// ktab_build for a policy whose second pool holds combs: the claimers store the entry's header
// and the 33 comb lines, and no window table.  Wave-uniform like ktab_build.
//   * entry 32 = A (affine after decompression), then the 16 bases 2^(16 m) A, m = 4 t + j, off
//     one chain of 240 doublings, parked as p3 points in entries 0..15 of the lane's table
//     workspace `at` (idle after a fast or balanced row);
//   * per block j: U+- = B[12+j] +- B[8+j], V+- = B[4+j] +- B[j] over the four bases' own
//     workspace entries, then the eight U +- V: 12 additions.  Complete formulas: every entry is
//     well defined for keys of small or mixed order (Z != 0; an entry may be the identity);
//   * Montgomery's trick over all 32: entry n waits in its own comb line as (X c, Y c, Z) with
//     c = Z_0 ... Z_(n-1), ONE inversion of the whole product, and the walk back turns line n
//     into the affine niels entry with (X c)(c Z_n)^-1, (Y c)(c Z_n)^-1.  A lane reads back only
//     lines it has stored itself; a lane that stores nothing computes on zeros.
// All comb lines and the header are stored before drain_release(), then the slot word.
template <class ATab, class KT>
NT_HD NT_INLINE void ktab_build_comb(const uint32_t Aw[8], uint32_t claim, const KT& kt, ATab& at) {
  static_assert(atab_entries_of<ATab>(0) >= kKcBases, "table workspace too small for the comb's bases");
  const uint32_t fp = ktab_fp(Aw);
  uint32_t idx = 0, have = 0;
  if (claim != kKtNoSlot) {
    idx = kt.pool_take();
    have = idx < kt.capacity() ? 1u : 0u;
    if (!have) kt.slot_store(claim, ktab_word(fp, kKtSeen));  // pool exhausted: seen for good
  }
  uint32_t flags, on;
  {
    ge_p3 P;
    const uint32_t ok = ge_frombytes_w(P, Aw);
    flags = (ok ? 0u : kKtUndecodable) | (ge_is_small_order_affine(P) ? kKtSmallOrder : 0u);
    on = have & ok;
    {
      fe one;
      fe_1(one);
      ge_niels q;
      ge_niels_from(q, P.X, P.Y, one);
      kc_line_put(kt, idx, kKcSigned, q, on);
    }
#pragma unroll 1
    for (uint32_t m = 0; m < kKcBases; ++m) {
      kc_park_p3(at, m, P);
      if (m + 1 < kKcBases) {
        ge_p2 q;
        ge_p3_to_p2(q, P);
#pragma unroll 1
        for (uint32_t r = 0; r + 1 < kKcCols; ++r) ge_dbl_p2(q, q);
        ge_cp c;
        ge_dbl(c, q);
        ge_cp_to_p3(P, c);
      }
    }
  }
  fe c;  // Z_0 ... Z_(n-1)
  fe_1(c);
#pragma unroll 1
  for (uint32_t j = 0; j < kKcBlocks; ++j) {
#pragma unroll 1
    for (uint32_t h = 0; h < 2; ++h) {  // h = 1: U+ -> 12 + j, U- -> 8 + j; h = 0: V+ -> 4 + j, V- -> j
      ge_p3 a, b, s, d;
      kc_take_p3(at, 8 * h + 4 + j, a);
      kc_take_p3(at, 8 * h + j, b);
      kc_add_sub(s, d, a, b);
      kc_park_p3(at, 8 * h + 4 + j, s);
      kc_park_p3(at, 8 * h + j, d);
    }
#pragma unroll 1
    for (uint32_t e = 0; e < kKcPerBlock; ++e) {
      // r2 = +1 (bit 2): U+, else U-.  (r1, r0) = ++: +V+, +-: +V-, -+: -V-, --: -V+
      const uint32_t lo = e & 3u;
      ge_p3 U, V;
      kc_take_p3(at, (e & 4u ? 12u : 8u) + j, U);
      kc_take_p3(at, (lo == 0u || lo == 3u ? 4u : 0u) + j, V);
      ge_cached vc;
      ge_p3_to_cached(vc, V);
      ge_cached_cneg(vc, lo < 2u ? 1u : 0u);
      ge_cp t;
      ge_add_cached(t, U, vc);
      ge_p2 r;
      ge_cp_to_p2(r, t);
      ge_niels w;
      fe_mul(w.ypx, r.X, c);
      fe_mul(w.ymx, r.Y, c);
      w.xy2d = r.Z;
      kc_line_put(kt, idx, kKcPerBlock * j + e, w, on);
      fe_mul(c, c, r.Z);
    }
  }
  fe inv;  // (Z_0 ... Z_n)^-1
  fe_invert_batch(inv, c);
#pragma unroll 1
  for (int n = (int)kKcSigned - 1; n >= 0; --n) {
    ge_niels w, q;
    kc_line_get(kt, idx, (uint32_t)n, w, on);
    ge_niels_from(q, w.ypx, w.ymx, inv);
    fe_mul(inv, inv, w.xy2d);
    kc_line_put(kt, idx, (uint32_t)n, q, on);
  }
  if (have) kt.hdr_store(idx, Aw, flags);
  // every storing wave drains and releases before any slot word names its entry
  kt.drain_release();
  if (have) kt.slot_publish(claim, ktab_word(fp, kKtReady0 + idx));
}

// The comb lookup of column col, block j (both wave-uniform): bit 16 j + col of each limb
// W_t (words 2 t, 2 t + 1 of the parked W), the top tooth's sign factored out.  Returns
// entry | negate << 8: the tables hold +A and the ladder sums -[K]A, so the entry is negated
// where the top tooth's bit is set.
template <class KT>
NT_HD NT_INLINE uint32_t kc_pick(const KT& kt, uint32_t col, uint32_t j) {
  const uint32_t w = j >> 1, sh = 16u * (j & 1u) + col;
  const uint32_t b3 = (kt.dig_get(6u + w) >> sh) & 1u;
  uint32_t e = 0;
#pragma unroll
  for (uint32_t t = 0; t < kKcTeeth - 1; ++t) e |= ((((kt.dig_get(2u * t + w) >> sh) & 1u) ^ b3) ^ 1u) << t;
  return (kKcPerBlock * j + e) | (b3 << 8);
}
// comb line `entry` of the key's entry kidx; off: the identity instead (the load still goes to
// an in-range line and is dropped)
template <class KT>
NT_HD NT_INLINE void kc_load(ge_niels& ne, const KT& kt, uint32_t kidx, uint32_t entry, uint32_t off) {
  kt.comb_load(kidx, entry, ne);
  ge_niels z;
  ge_niels_0(z);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    ne.ypx.v[i] = off ? z.ypx.v[i] : ne.ypx.v[i];
    ne.ymx.v[i] = off ? z.ymx.v[i] : ne.ymx.v[i];
    ne.xy2d.v[i] = off ? z.xy2d.v[i] : ne.xy2d.v[i];
  }
}

// The comb's recoding of the full hash scalar k < L: K = k | 1, W = (K >> 1) | 2^255 (k < 2^253:
// bit 255 is free).  The 8 words of W wait with kt.dig_put / dig_get as ladder_k4's digits do
// (the kernel: LDS), word 8 holds c = 1 - (k & 1).
template <class KT>
NT_HD NT_INLINE void kc_recode(const uint32_t k[8], const KT& kt) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t lo = i == 0 ? (k[0] | 1u) : k[i];
    kt.dig_put((uint32_t)i, (lo >> 1) | (i < 7 ? k[i + 1] << 31 : 0x80000000u));
  }
  kt.dig_put(8u, (k[0] & 1u) ^ 1u);
}
// t = [k](-A) (completed) for the full k < L from the key's comb (pool entry kidx's lines of
// the second pool; dead: the key has no comb, every lookup is the identity): 64 lookups, 15
// doublings, 64 mixed additions and the parity's correction, nothing of R and no lattice vector.
// Columns 15 .. 0, one doubling before each but the first (from the completed point:
// ge_cp_to_p2 + ge_dbl), blocks 0 .. 3 within a column; the first lookup seeds the accumulator;
// the last addition, executed by every lane, is +A where c = 1 (-[K]A + A = -[k]A) and the
// identity where c = 0.  The next entry's load is issued right after the multiplies that consume
// the current one, one ahead and no further, as in wcomb_acc.  Column and block are wave-uniform:
// nothing is indexed per lane.
template <class KT>
NT_HD NT_INLINE void ladder_kc(ge_cp& t, const uint32_t k[8], uint32_t dead, const KT& kt, uint32_t kidx) {
  kc_recode(k, kt);
  constexpr uint32_t kTop = kKcCols - 1;
  uint32_t pk = kc_pick(kt, kTop, 0u);
  ge_niels ne;
  kc_load(ne, kt, kidx, pk & 0xffu, dead);
  ge_niels_cneg(ne, pk >> 8);
  ge_p3 acc;
  ge_p3_from_niels(acc, ne);
  pk = kc_pick(kt, kTop, 1u);
  kc_load(ne, kt, kidx, pk & 0xffu, dead);
#pragma unroll 1
  for (uint32_t col = kTop + 1; col-- > 0;) {
    if (col != kTop) {
      ge_p2 q;
      ge_cp_to_p2(q, t);
      ge_dbl(t, q);
    }
#pragma unroll 1
    for (uint32_t j = col == kTop ? 1u : 0u; j < kKcBlocks; ++j) {
      if (col != kTop || j != 1u) ge_cp_to_p3(acc, t);
      ge_niels_cneg(ne, pk >> 8);
      fe PP, MM, TT;
      ge_add_niels_1(PP, MM, TT, acc, ne);
      if (j + 1 < kKcBlocks || col != 0) {
        pk = j + 1 < kKcBlocks ? kc_pick(kt, col, j + 1) : kc_pick(kt, col - 1, 0u);
        kc_load(ne, kt, kidx, pk & 0xffu, dead);
      } else {
        // the correction: +A, never negated
        kc_load(ne, kt, kidx, kKcSigned, dead | (kt.dig_get(8u) ^ 1u));
      }
      ge_add_niels_2(t, PP, MM, TT, acc.Z);
    }
  }
  ge_cp_to_p3(acc, t);
  ge_add_niels(t, acc, ne);
}

// verify_k4 over the key's comb instead of its four tables: the same verdict for every input
// (ladder_kc's sum is [k](-A) as an integer identity), everything after the ladder unchanged.
template <int MODE, class WComb, class KT>
NT_HD NT_INLINE uint32_t verify_kc(const uint32_t Rw[8], const uint32_t Sw[8], const uint32_t k[8], uint32_t kflags,
                                   const WComb& wb, const KT& kt, uint32_t kidx) {
  const uint32_t dead = (kflags & kKtUndecodable) ? 1u : 0u;
  uint32_t ok = sc_is_canonical(Sw) & (dead ^ 1u);
  if (MODE == kStrict) ok &= (kflags & kKtSmallOrder) ? 0u : 1u;
  ge_cp t;
  ladder_kc(t, k, dead, kt, kidx);
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
