// nt_probe_items.hpp -- TEST INFRASTRUCTURE: item i of every arithmetic probe,
// written once and run two ways: by one GPU thread each in nt_device_probe.hip
// (the gfx950 build of narwhal-tusk_amd/csrc/*.hpp) and in a loop by
// nt_host_harness.cpp (the same headers compiled by g++).  Each function is a
// thin wrapper: it moves item i's words in and out of flat arrays and calls the
// header function under test; no arithmetic lives here.  The entry points around
// the items are written once too (nt_probe_entries.inc); how they describe an item's
// arguments to the two runners is at the end of this file.
// Field elements are 10 limbs, encodings and scalars 8 little-endian words.
#pragma once
#include <type_traits>

#include "../../narwhal-tusk_amd/csrc/ed25519_ops.hpp"
#include "../../narwhal-tusk_amd/csrc/fe_inv_vt.hpp"
#include "../../narwhal-tusk_amd/csrc/wcomb_build.hpp"

namespace ntp {
using namespace nt;

NT_HD NT_INLINE void ld_fe(fe& a, const uint32_t* p, size_t i) {
#pragma unroll
  for (int l = 0; l < 10; ++l) a.v[l] = p[10 * i + l];
}
NT_HD NT_INLINE void st_fe(uint32_t* p, size_t i, const fe& a) {
#pragma unroll
  for (int l = 0; l < 10; ++l) p[10 * i + l] = a.v[l];
}
template <int N>
NT_HD NT_INLINE void ld_w(uint32_t* w, const uint32_t* p, size_t i) {
#pragma unroll
  for (int l = 0; l < N; ++l) w[l] = p[N * i + l];
}
template <int N>
NT_HD NT_INLINE void st_w(uint32_t* p, size_t i, const uint32_t* w) {
#pragma unroll
  for (int l = 0; l < N; ++l) p[N * i + l] = w[l];
}

NT_HD NT_INLINE void item_fe_mul(size_t i, const uint32_t* f, const uint32_t* g, uint32_t* out) {
  fe a, b, c;
  ld_fe(a, f, i);
  ld_fe(b, g, i);
  fe_mul(c, a, b);
  st_fe(out, i, c);
}
NT_HD NT_INLINE void item_fe_sq(size_t i, const uint32_t* f, uint32_t* out) {
  fe a, c;
  ld_fe(a, f, i);
  fe_sq(c, a);
  st_fe(out, i, c);
}
NT_HD NT_INLINE void item_fe_sq_wide(size_t i, const uint32_t* f, uint32_t* out) {
  fe a, c;
  ld_fe(a, f, i);
  fe_sq_wide(c, a);
  st_fe(out, i, c);
}
NT_HD NT_INLINE void item_fe_carry(size_t i, const uint32_t* f, uint32_t* out) {
  fe a;
  ld_fe(a, f, i);
  fe_carry(a);
  st_fe(out, i, a);
}
NT_HD NT_INLINE void item_fe_tobytes(size_t i, const uint32_t* f, uint32_t* out8) {
  fe a;
  ld_fe(a, f, i);
  uint32_t w[8];
  fe_tobytes_w(w, a);
  st_w<8>(out8, i, w);
}
NT_HD NT_INLINE void item_fe_frombytes(size_t i, const uint32_t* in8, uint32_t* out) {
  uint32_t w[8];
  ld_w<8>(w, in8, i);
  fe a;
  fe_frombytes_w(a, w);
  st_fe(out, i, a);
}
// vt: fe_invert_vt (binary GCD), else fe_invert (Fermat); canonical words out
NT_HD NT_INLINE void item_fe_invert(size_t i, const uint32_t* f, uint32_t* out8, int vt) {
  fe a, r;
  ld_fe(a, f, i);
  if (vt) fe_invert_vt(r, a);
  else fe_invert(r, a);
  uint32_t w[8];
  fe_tobytes_w(w, r);
  st_w<8>(out8, i, w);
}
NT_HD NT_INLINE void item_sc_reduce512(size_t i, const uint32_t* in16, uint32_t* out8) {
  uint32_t x[16], r[8];
  ld_w<16>(x, in16, i);
  sc_reduce512(r, x);
  st_w<8>(out8, i, r);
}
NT_HD NT_INLINE void item_sc_muladd(size_t i, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                    uint32_t* out8) {
  uint32_t wa[8], wb[8], wc[8], r[8];
  ld_w<8>(wa, a, i);
  ld_w<8>(wb, b, i);
  ld_w<8>(wc, c, i);
  sc_muladd(r, wa, wb, wc);
  st_w<8>(out8, i, r);
}
NT_HD NT_INLINE void item_sc_mul(size_t i, const uint32_t* a, const uint32_t* b, uint32_t* out8) {
  uint32_t wa[8], wb[8], r[8];
  ld_w<8>(wa, a, i);
  ld_w<8>(wb, b, i);
  sc_mul(r, wa, wb);
  st_w<8>(out8, i, r);
}
// out8 = |k'|, neg[i] = 1 iff k' = k - L was taken
NT_HD NT_INLINE void item_sc_reduce_half(size_t i, const uint32_t* k8, uint32_t* out8, uint32_t* neg) {
  uint32_t k[8];
  ld_w<8>(k, k8, i);
  neg[i] = sc_reduce_half(k);
  st_w<8>(out8, i, k);
}
NT_HD NT_INLINE void item_sc_recode_w4(size_t i, const uint32_t* s8, uint32_t* out8) {
  uint32_t s[8], d[8];
  ld_w<8>(s, s8, i);
  sc_recode_w4(d, s);
  st_w<8>(out8, i, d);
}
NT_HD NT_INLINE void item_sc_is_canonical(size_t i, const uint32_t* s8, uint32_t* out1) {
  uint32_t s[8];
  ld_w<8>(s, s8, i);
  out1[i] = sc_is_canonical(s);
}
// sc_halfsize_t<lehmer>: u, v (8 words), sign of u, bits
NT_HD NT_INLINE void item_sc_halfsize(size_t i, const uint32_t* k8, uint32_t* u8, uint32_t* uneg, uint32_t* v8,
                                      int32_t* bits, int lehmer) {
  uint32_t k[8], u[8], v[8], un;
  ld_w<8>(k, k8, i);
  bits[i] = lehmer ? sc_halfsize_t<true>(u, un, v, k) : sc_halfsize_t<false>(u, un, v, k);
  uneg[i] = un;
  st_w<8>(u8, i, u);
  st_w<8>(v8, i, v);
}
// k = H(R || A || M) mod L, M = msg[off[i] .. off[i] + len[i]) at whatever alignment that is
NT_HD NT_INLINE void item_hram(size_t i, const uint32_t* R8, const uint32_t* A8, const uint8_t* msg,
                               const uint64_t* off, const uint64_t* len, uint32_t* out8, int fast) {
  uint32_t R[8], A[8], k[8];
  ld_w<8>(R, R8, i);
  ld_w<8>(A, A8, i);
  if (fast) hram_scalar<true>(k, R, A, msg + off[i], len[i]);
  else hram_scalar<false>(k, R, A, msg + off[i], len[i]);
  st_w<8>(out8, i, k);
}
// out4 = decodes, [8]P == 0 by doublings, torsion-y compare of the decoded point,
// torsion_y_words on the canonical y of the encoding
NT_HD NT_INLINE void item_point_checks(size_t i, const uint32_t* enc8, uint32_t* out4) {
  uint32_t w[8], y[8];
  ld_w<8>(w, enc8, i);
  ge_p3 P;
  out4[4 * i] = ge_frombytes_w(P, w);
  out4[4 * i + 1] = ge_is_small_order(P);
  out4[4 * i + 2] = ge_is_small_order_affine(P);
  fe_tobytes_w(y, P.Y);
  out4[4 * i + 3] = torsion_y_words(y);
}
// verify_uv's variable-base part: -[u]A - [v]R through the lane's tables, every
// lane of a wave running its wave's largest window count; out8 = the encoding
template <class ATab>
NT_HD NT_INLINE void item_ladder_uv(size_t i, const uint32_t* A8, const uint32_t* R8, const uint32_t* u8,
                                    const uint32_t* uneg, const uint32_t* v8, const int32_t* bits, ATab& at,
                                    uint32_t* out8, bool write) {
  uint32_t Aw[8], Rw[8], u[8], v[8], ud[8], vd[8], o[8];
  ld_w<8>(Aw, A8, i);
  ld_w<8>(Rw, R8, i);
  ld_w<8>(u, u8, i);
  ld_w<8>(v, v8, i);
  {
    ge_p3 A;
    ge_frombytes_w(A, Aw);
    ptab_build(A, uneg[i] ^ 1u, at, 0);
  }
  {
    ge_p3 R;
    ge_frombytes_w(R, Rw);
    ptab_build(R, 1u, at, kTabR);
  }
  sc_recode_w4(ud, u);
  sc_recode_w4(vd, v);
  const int W = wave_max((bits[i] + 5) >> 2);
  ge_cp t;
  ladder_ar(t, ud, vd, W, at);
  ge_p2 p;
  ge_cp_to_p2(p, t);
  ge_tobytes_w(o, p);
  if (write) st_w<8>(out8, i, o);
}

// sc_unbalanced_t<lehmer>: u, v (8 words), sign of u, bit lengths of |u| and v
NT_HD NT_INLINE void item_sc_unbalanced(size_t i, const uint32_t* k8, uint32_t* u8, uint32_t* uneg, uint32_t* v8,
                                        int32_t* ubits, int32_t* vbits, int lehmer) {
  uint32_t k[8], u[8], v[8], un;
  int ub, vb;
  ld_w<8>(k, k8, i);
  if (lehmer) sc_unbalanced_t<true>(u, un, v, k, ub, vb);
  else sc_unbalanced_t<false>(u, un, v, k, ub, vb);
  uneg[i] = un;
  ubits[i] = ub;
  vbits[i] = vb;
  st_w<8>(u8, i, u);
  st_w<8>(v8, i, v);
}

// The key-table cache items run over one flat allocation laid out as DevKTab
// (kernels_common.hpp) reads it: a 128-byte control block, kKtProbeSlots index
// slots of 8 bytes, then `capacity` pool entries of kKtEntryBytes.
constexpr uint32_t kKtProbeSlots = 4096, kKtProbeCtlBytes = 128;
constexpr size_t kKtProbePoolOff = kKtProbeCtlBytes + 8 * (size_t)kKtProbeSlots;
constexpr uint32_t kKtProbeMaxCap = 1u << 12;
inline size_t ktab_probe_bytes(uint32_t capacity) { return kKtProbePoolOff + (size_t)capacity * kKtEntryBytes; }
// the entry points' argument checks, on the host before anything runs: table and digit of
// every ktab_point item, entry index (below the capacity), flags and bit lengths of every
// ladder_uv3 item
inline bool ktab_point_args_ok(uint64_t n, const int32_t* td2) {
  for (uint64_t i = 0; i < n; ++i)
    if (td2[2 * i] < 0 || td2[2 * i] >= (int32_t)kKtTables || td2[2 * i + 1] < -8 || td2[2 * i + 1] > 8) return false;
  return true;
}
inline bool ladder_uv3_args_ok(uint64_t n, const uint32_t* kidx, const uint32_t* sc4, uint32_t capacity) {
  for (uint64_t i = 0; i < n; ++i)
    if (kidx[i] >= capacity || sc4[4 * i] > 1u || sc4[4 * i + 1] > 253u || sc4[4 * i + 2] > 253u || sc4[4 * i + 3] > 1u)
      return false;
  return true;
}

// The table of item i's key as verify_n makes it: ktab_probe -> ktab_take -> ktab_build.
// live = false (a lane past n): no probe, no claim, ktab_build's arithmetic alone.
// slot[i] = the index slot won, or kKtNoSlot.
template <class KT>
NT_HD NT_INLINE void item_ktab_fill(size_t i, const uint32_t* A8, const KT& kt, uint32_t* slot, bool live) {
  uint32_t Aw[8];
  ld_w<8>(Aw, A8, i);
  uint32_t claim = kKtNoSlot;
  if (live) {
    KtProbe p;
    ktab_probe(p, Aw, kt);
    claim = ktab_take(p, kt);
  }
  ktab_build(Aw, claim, kt);
  if (live) slot[i] = claim;
}
// What a reader finds for item i's key: out3 = entry index (kKtNoSlot: not ready), tag
// match, header flags; enc8 = the encoding of the cached point tab_load_signed(idx, t, d)
// hands out for (t, d) = td2[2 i], td2[2 i + 1], added to the identity.
template <class KT>
NT_HD NT_INLINE void item_ktab_point(size_t i, const uint32_t* A8, const int32_t* td2, const KT& kt, uint32_t* out3,
                                     uint32_t* enc8) {
  uint32_t Aw[8], o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  ld_w<8>(Aw, A8, i);
  KtProbe p;
  ktab_probe(p, Aw, kt);
  const uint32_t idx = ktab_ready_index(p, kt);
  uint32_t same = 0, flags = 0;
  if (idx != kKtNoSlot) {
    kt.acquire();
    uint32_t tag[8];
    kt.hdr_load(idx, tag, flags);
    same = 1;
#pragma unroll
    for (int l = 0; l < 8; ++l) same &= tag[l] == Aw[l];
    ge_cached ce;
    kt.tab_load_signed(idx, (uint32_t)td2[2 * i], td2[2 * i + 1], ce);
    ge_p3 id;
    ge_p3_0(id);
    ge_cp c;
    ge_add_cached(c, id, ce);
    ge_p2 q;
    ge_cp_to_p2(q, c);
    ge_tobytes_w(o, q);
  }
  out3[3 * i] = idx;
  out3[3 * i + 1] = same;
  out3[3 * i + 2] = flags;
  st_w<8>(enc8, i, o);
}
// verify_uv3's variable-base part: -[u]A - [v]R from the cached tables of pool entry
// kidx[i] and the lane's own table of -R (ladder_uv3: the recoding, the window rule,
// wave_max and ladder_a3r); sc4 = uneg, ubits, vbits, dead per item
template <class ATab, class KT>
NT_HD NT_INLINE void item_ladder_uv3(size_t i, const uint32_t* kidx, const uint32_t* R8, const uint32_t* u8,
                                     const uint32_t* v8, const uint32_t* sc4, ATab& at, const KT& kt, uint32_t* out8,
                                     bool write) {
  uint32_t Rw[8], u[8], v[8], o[8];
  ld_w<8>(Rw, R8, i);
  ld_w<8>(u, u8, i);
  ld_w<8>(v, v8, i);
  {
    ge_p3 R;
    ge_frombytes_w(R, Rw);
    ptab_build(R, 1u, at, kTabR);
  }
  ge_cp t;
  ladder_uv3(t, u, sc4[4 * i], v, (int)sc4[4 * i + 1], (int)sc4[4 * i + 2], sc4[4 * i + 3], at, kt, kidx[i]);
  ge_p2 p;
  ge_cp_to_p2(p, t);
  ge_tobytes_w(o, p);
  if (write) st_w<8>(out8, i, o);
}

// ---- the key-table cache's comb path (ktab_comb.hpp ktab_build_comb, kc_recode / kc_pick,
// ladder_kc, verify_kc; ed25519_ops.hpp compare_one).  These items run over a second layout: the blob above,
// words 8..9 of its control block carrying the comb pool's address, then `capacity` combs of
// kKtCombBytes, then kKcProbeGuardBytes that nothing may write (the caller prefills pool, combs
// and guard and reads them back).  The three-table items above keep their blob (words 8..9
// zero: has_comb() is false there and the window tables are built).
constexpr size_t kKcProbeGuardBytes = 8192;
constexpr int kKcPickWords = 65;  // per item of the picks probe: 64 lookups, then c
inline size_t kcomb_probe_comb_off(uint32_t capacity) { return ktab_probe_bytes(capacity); }
inline size_t kcomb_probe_bytes(uint32_t capacity) {
  return kcomb_probe_comb_off(capacity) + (size_t)capacity * kKtCombBytes + kKcProbeGuardBytes;
}
static_assert(kKtProbePoolOff % 128 == 0 && kKtEntryBytes % 128 == 0 && kKtCombBytes % 128 == 0,
              "the comb pool starts on a 128-byte line of the blob");
// the entry points' argument checks, on the host before anything runs
inline bool kcomb_cap_ok(uint32_t capacity) { return capacity >= 1 && capacity <= kKtProbeMaxCap; }
inline bool kc_scalars_ok(uint64_t n, const uint32_t* k8) {  // k < 2^253: bit 255 of W is free
  for (uint64_t i = 0; i < n; ++i)
    if (k8[8 * i + 7] >> 29) return false;
  return true;
}
inline bool ladder_kc_args_ok(uint64_t n, const uint32_t* kidx, const uint32_t* k8, const uint32_t* dead,
                              uint32_t capacity) {
  for (uint64_t i = 0; i < n; ++i)
    if (kidx[i] >= capacity || dead[i] > 1u) return false;
  return kc_scalars_ok(n, k8);
}
inline bool modes_ok(uint64_t n, const uint32_t* mode) {
  for (uint64_t i = 0; i < n; ++i)
    if (mode[i] > 1u) return false;
  return true;
}
inline bool verify_kc_args_ok(uint64_t n, const uint32_t* kidx, const uint32_t* kflags, const uint32_t* k8,
                              const uint32_t* mode, uint32_t capacity) {
  for (uint64_t i = 0; i < n; ++i)
    if (kidx[i] >= capacity || kflags[i] > (kKtUndecodable | kKtSmallOrder)) return false;
  return kc_scalars_ok(n, k8) && modes_ok(n, mode);
}

// The comb of item i's key as verify_n makes it: ktab_probe -> ktab_take -> the four-argument
// ktab_build with the lane's table workspace.  live = false (a lane past n): no probe, no
// claim, the build's arithmetic alone.  slot[i] = the index slot won, or kKtNoSlot.
template <class ATab, class KT>
NT_HD NT_INLINE void item_kcomb_fill(size_t i, const uint32_t* A8, const KT& kt, ATab& at, uint32_t* slot, bool live) {
  uint32_t Aw[8];
  ld_w<8>(Aw, A8, i);
  uint32_t claim = kKtNoSlot;
  if (live) {
    KtProbe p;
    ktab_probe(p, Aw, kt);
    claim = ktab_take(p, kt);
  }
  ktab_build(Aw, claim, kt, at);
  if (live) slot[i] = claim;
}
// What a reader finds for item i's key: out3 as item_ktab_point's; limbs30 = comb line
// line[i] of the key's entry through comb_load (a number past 32 goes through comb_line's clamp)
template <class KT>
NT_HD NT_INLINE void item_kcomb_line(size_t i, const uint32_t* A8, const uint32_t* line, const KT& kt, uint32_t* out3,
                                     uint32_t* limbs30) {
  uint32_t Aw[8];
  ld_w<8>(Aw, A8, i);
  KtProbe p;
  ktab_probe(p, Aw, kt);
  const uint32_t idx = ktab_ready_index(p, kt);
  uint32_t same = 0, flags = 0;
  ge_niels q;
  fe_0(q.ypx); fe_0(q.ymx); fe_0(q.xy2d);
  if (idx != kKtNoSlot) {
    kt.acquire();
    uint32_t tag[8];
    kt.hdr_load(idx, tag, flags);
    same = 1;
#pragma unroll
    for (int l = 0; l < 8; ++l) same &= tag[l] == Aw[l];
    kt.comb_load(idx, line[i], q);
  }
  out3[3 * i] = idx;
  out3[3 * i + 1] = same;
  out3[3 * i + 2] = flags;
  uint32_t* o = limbs30 + 30 * i;
#pragma unroll
  for (int l = 0; l < 10; ++l) { o[l] = q.ypx.v[l]; o[10 + l] = q.ymx.v[l]; o[20 + l] = q.xy2d.v[l]; }
}
// kc_recode of k, then the 64 kc_pick words (entry | negate << 8) in ladder_kc's order --
// columns 15 .. 0, blocks 0 .. 3 within a column -- and c; the parked W goes through
// kt.dig_put / dig_get (the device: the LDS digit cells)
template <class KT>
NT_HD NT_INLINE void item_kc_picks(size_t i, const uint32_t* k8, const KT& kt, uint32_t* out65) {
  uint32_t k[8];
  ld_w<8>(k, k8, i);
  kc_recode(k, kt);
  uint32_t* o = out65 + (size_t)kKcPickWords * i;
  int n = 0;
  for (uint32_t col = kKcCols; col-- > 0;)
    for (uint32_t j = 0; j < kKcBlocks; ++j) o[n++] = kc_pick(kt, col, j);
  o[n] = kt.dig_get(8u);
}
// ladder_kc's [k](-A) over the comb of pool entry kidx[i] (dead[i]: the identity); out8 = the encoding
template <class KT>
NT_HD NT_INLINE void item_ladder_kc(size_t i, const uint32_t* kidx, const uint32_t* k8, const uint32_t* dead,
                                    const KT& kt, uint32_t* out8, bool write) {
  uint32_t k[8], o[8];
  ld_w<8>(k, k8, i);
  ge_cp t;
  ladder_kc(t, k, dead[i], kt, kidx[i]);
  ge_p2 p;
  ge_cp_to_p2(p, t);
  ge_tobytes_w(o, p);
  if (write) st_w<8>(out8, i, o);
}
// compare_one<MODE> of R' = (x z : y z : z) with the encoding R (x, y, z: 8 words each, taken as
// fe_frombytes_w takes them; z != 0), z inverted by fe_invert_batch, the strict small-order
// test as verify_kc asks for it; mode 0 strict, 1 cofactorless
NT_HD NT_INLINE void item_compare_one(size_t i, const uint32_t* x8, const uint32_t* y8, const uint32_t* z8,
                                      const uint32_t* R8, const uint32_t* mode, uint32_t* out1) {
  uint32_t xw[8], yw[8], zw[8], Rw[8];
  ld_w<8>(xw, x8, i);
  ld_w<8>(yw, y8, i);
  ld_w<8>(zw, z8, i);
  ld_w<8>(Rw, R8, i);
  fe x, y, z, zi;
  fe_frombytes_w(x, xw);
  fe_frombytes_w(y, yw);
  fe_frombytes_w(z, zw);
  ge_p2 P;
  fe_mul(P.X, x, z);
  fe_mul(P.Y, y, z);
  P.Z = z;
  fe_invert_batch(zi, z);
  out1[i] = mode[i] == 0 ? compare_one<kStrict>(P, zi, Rw, true) : compare_one<kCofactorless>(P, zi, Rw, false);
}
// verify_kc's bit for (R, S, k) over the comb of pool entry kidx[i], the header flags as given, wb the comb of B
template <class WComb, class KT>
NT_HD NT_INLINE void item_verify_kc(size_t i, const uint32_t* kidx, const uint32_t* kflags, const uint32_t* R8,
                                    const uint32_t* S8, const uint32_t* k8, const uint32_t* mode, const WComb& wb,
                                    const KT& kt, uint32_t* out1, bool write) {
  uint32_t Rw[8], Sw[8], k[8];
  ld_w<8>(Rw, R8, i);
  ld_w<8>(Sw, S8, i);
  ld_w<8>(k, k8, i);
  const uint32_t ok = mode[i] == 0 ? verify_kc<kStrict>(Rw, Sw, k, kflags[i], wb, kt, kidx[i])
                                   : verify_kc<kCofactorless>(Rw, Sw, k, kflags[i], wb, kt, kidx[i]);
  if (write) out1[i] = ok;
}

// ---- the wide combs (ed25519_ops.hpp wcomb_*, wcomb_build.hpp): digits, table entries, sums.
// A comb type here is the product's WideComb<W> (device), or a host type with the same
// members: kBits, base, load, load_corr.
constexpr uint32_t kWcCorrIdx = 0xffffffffu;  // "the [L]P entry" where an entry index is expected
constexpr uint32_t kWcMaxKeys = 8;            // keys of one probe comb set
constexpr size_t kWcGuardBytes = 8192;        // the pattern that follows the combs
constexpr int kWcFill = 0xA5;                 // ... and fills them before the build
constexpr int kWcMaxLoads = 17;               // kPos + 1 of the narrowest comb: wcomb_acc's loads
constexpr int kWcDigitWords = 64;             // words per item of the digits probe

// bits -> f(std::integral_constant<int, W>); false: not one of the five widths
template <class F>
inline bool wcomb_width(int bits, F&& f) {
  switch (bits) {
    case kKeyCombNarrow: f(std::integral_constant<int, kKeyCombNarrow>{}); return true;
    case kKeyCombMid: f(std::integral_constant<int, kKeyCombMid>{}); return true;
    case kKeyCombWide: f(std::integral_constant<int, kKeyCombWide>{}); return true;
    case kKeyCombReduced: f(std::integral_constant<int, kKeyCombReduced>{}); return true;
    case kBCombBits: f(std::integral_constant<int, kBCombBits>{}); return true;
    default: return false;
  }
}

// The digits wcomb_acc takes from x, in its order: digit j < kPos belongs to position j (the
// last one of a reduced comb unsigned), digit kPos is the one behind the last round's reload.
template <int W>
NT_HD NT_INLINE void wcomb_schedule(int32_t dg[kWcMaxLoads], const uint32_t x[8]) {
  constexpr int P = CombGeom<W>::kPos;
  uint32_t d[8], carry = 0;
#pragma unroll
  for (int m = 0; m < 8; ++m) d[m] = x[m];
  for (int j = 0; j <= P; ++j) dg[j] = wcomb_digit<W>(d, carry, CombGeom<W>::kReduced && j == P - 1);
}
// every table index wcomb_acc forms for x lies inside a position's kEntries
template <int W>
inline bool wcomb_scalar_ok(const uint32_t x[8]) {
  int32_t dg[kWcMaxLoads];
  wcomb_schedule<W>(dg, x);
  for (int j = 0; j <= CombGeom<W>::kPos; ++j)
    if ((dg[j] < 0 ? -dg[j] : dg[j]) >= CombGeom<W>::kEntries) return false;
  return true;
}
// A comb that reads nothing: it notes (position, index) of every load wcomb_acc issues, in
// order, at rec[1 ..] and their count at rec[0], and hands back the identity.
template <int W>
struct RecordingComb {
  static constexpr int kBits = W;
  uint32_t* rec;
  NT_HD NT_INLINE void load(uint32_t pos, uint32_t idx, ge_niels& q) const {
    const uint32_t c = rec[0];
    if (c < (uint32_t)kWcMaxLoads) {
      rec[1 + 2 * c] = pos;
      rec[2 + 2 * c] = idx;
    }
    rec[0] = c + 1;
    ge_niels_0(q);
  }
  NT_HD NT_INLINE void load_corr(ge_niels& q) const { ge_niels_0(q); }
};
// out (kWcDigitWords per item): words 0 .. kPos the schedule's signed digits; word 17 the
// number of loads wcomb_acc itself issued for x and from word 18 on their (position, index)
template <int W>
NT_HD NT_INLINE void item_wcomb_digits(size_t i, const uint32_t* x8, uint32_t* out) {
  uint32_t x[8];
  ld_w<8>(x, x8, i);
  uint32_t* o = out + (size_t)kWcDigitWords * i;
  int32_t dg[kWcMaxLoads];
  wcomb_schedule<W>(dg, x);
  for (int j = 0; j < kWcDigitWords; ++j) o[j] = 0;
  for (int j = 0; j <= CombGeom<W>::kPos; ++j) o[j] = (uint32_t)dg[j];
  ge_p3 acc;
  wcomb_acc<RecordingComb<W>, true>(acc, x, RecordingComb<W>{o + kWcMaxLoads});
}
// entry (pos, idx) of the comb through load (idx = kWcCorrIdx: load_corr): the 30 limbs, then
// words 30 and 31 of the entry as they lie in memory
template <class Comb>
NT_HD NT_INLINE void item_wcomb_entry(size_t i, const Comb& wc, uint32_t pos, uint32_t idx, uint32_t* out32) {
  using G = CombGeom<Comb::kBits>;
  ge_niels q;
  size_t word;
  if (idx == kWcCorrIdx) {
    wc.load_corr(q);
    word = G::kCorrWord;
  } else {
    wc.load(pos, idx, q);
    word = ((size_t)pos * G::kEntries + idx) * kWStride;
  }
  uint32_t* o = out32 + 32 * i;
#pragma unroll
  for (int l = 0; l < 10; ++l) { o[l] = q.ypx.v[l]; o[10 + l] = q.ymx.v[l]; o[20 + l] = q.xy2d.v[l]; }
  o[30] = wc.base[word + 30];
  o[31] = wc.base[word + 31];
}
NT_HD NT_INLINE void st_point(uint32_t* out8, size_t i, const ge_p3& P) {
  ge_p2 p;
  ge_p3_to_p2(p, P);
  uint32_t o[8];
  ge_tobytes_w(o, p);
  st_w<8>(out8, i, o);
}
// out = start + [+-x]P through wcomb_acc; flags bit 0: kFromIdentity (start unused), bit 1:
// neg_all.  A start that does not decode counts as the identity.
template <class Comb>
NT_HD NT_INLINE void item_wcomb_acc(size_t i, const Comb& wc, const uint32_t* x8, const uint32_t* flags,
                                    const uint32_t* start8, uint32_t* out8) {
  uint32_t x[8], s[8];
  ld_w<8>(x, x8, i);
  ld_w<8>(s, start8, i);
  const uint32_t neg = (flags[i] >> 1) & 1u;
  ge_p3 acc;
  if (flags[i] & 1u) {
    wcomb_acc<Comb, true>(acc, x, wc, neg);
  } else {
    if (!ge_frombytes_w(acc, s)) ge_p3_0(acc);
    wcomb_acc<Comb, false>(acc, x, wc, neg);
  }
  st_point(out8, i, acc);
}
// [k](-A) as cached_point forms it from the key's comb: key_comb_sum
template <class Comb>
NT_HD NT_INLINE void item_key_comb_sum(size_t i, const Comb& wc, const uint32_t* meta, const uint32_t* k8,
                                       uint32_t* out8) {
  uint32_t k[8];
  ld_w<8>(k, k8, i);
  ge_p3 acc;
  key_comb_sum(acc, k, meta[i], wc);
  st_point(out8, i, acc);
}
// the scalar key_comb_sum hands to wcomb_acc keeps inside the table
template <int W>
inline bool key_comb_scalar_ok(const uint32_t k8[8]) {
  uint32_t k[8];
  for (int m = 0; m < 8; ++m) k[m] = k8[m];
  if (CombGeom<W>::kReduced) (void)sc_reduce_half(k);
  return wcomb_scalar_ok<W>(k);
}
// the argument checks of the comb entry points, on the host before anything runs
template <int W>
inline bool wcomb_entry_args_ok(uint64_t n, uint32_t nkeys, const uint32_t* key, const uint32_t* pos,
                                const uint32_t* idx) {
  using G = CombGeom<W>;
  for (uint64_t i = 0; i < n; ++i) {
    if (key[i] >= nkeys) return false;
    if (idx[i] == kWcCorrIdx ? !G::kReduced : (pos[i] >= (uint32_t)G::kPos || idx[i] >= (uint32_t)G::kEntries)) return false;
  }
  return true;
}
template <int W>
inline bool wcomb_acc_args_ok(uint64_t n, uint32_t nkeys, const uint32_t* key, const uint32_t* x8,
                              const uint32_t* flags) {
  for (uint64_t i = 0; i < n; ++i)
    if (key[i] >= nkeys || flags[i] > 3u || !wcomb_scalar_ok<W>(x8 + 8 * i)) return false;
  return true;
}
template <int W>
inline bool key_comb_args_ok(uint64_t n, uint32_t nkeys, const uint32_t* key, const uint32_t* k8) {
  for (uint64_t i = 0; i < n; ++i)
    if (key[i] >= nkeys || !key_comb_scalar_ok<W>(k8 + 8 * i)) return false;
  return true;
}
// what a comb set may be: one of the five widths; the 24-bit comb for one point, not negated
// (the product builds it for B alone); at most kWcMaxKeys keys; a batch of at least one key
inline bool wcomb_build_args_ok(int bits, uint32_t nkeys, int negate, uint32_t batch) {
  if (!wcomb_width(bits, [](auto) {})) return false;
  if (nkeys < 1 || nkeys > kWcMaxKeys || batch < 1) return false;
  return bits != kBCombBits || (nkeys == 1 && !negate);
}

// ---- how an entry point (nt_probe_entries.inc) describes item i's arguments to its runner's
// run<Tail>(n, item, args...): the arguments stand in the item's own order, and each runner
// (nt_device_probe.hip, nt_host_harness.cpp) turns a description into what its items take.
// Anything that is none of the descriptions below goes to the item as it is.
struct Leave {};   // lanes past n leave at once
struct Repeat {};  // lanes past n run item n - 1 with false for the item's trailing bool: they write nothing
template <class T>
struct In {  // the caller's input, `bytes` per item
  const T* p;
  size_t bytes;
};
template <class T>
struct Out {  // the caller's output, `bytes` per item
  T* p;
  size_t bytes;
};
template <class T>
inline In<T> in(const T* p, size_t bytes) { return {p, bytes}; }
template <class T>
inline Out<T> out_(T* p, size_t bytes) { return {p, bytes}; }
struct Ws {};  // the lane's [k]A table workspace
template <bool COMB>
struct Blob {  // the caller's key table of `cap` entries, read and written; COMB: with the comb pool and guard
  uint8_t* p;
  uint32_t cap;
  size_t bytes() const { return COMB ? kcomb_probe_bytes(cap) : ktab_probe_bytes(cap); }
};
struct NoTable {};  // the key-table policy with no table behind it: its digit cells alone
struct Msg {        // hram's message buffer: the items get a zero-padded, aligned copy
  const uint8_t* p;
  uint64_t bytes;
};
// a run-time switch as a compile-time constant: the items' int arguments fold, a width selects the template
template <int V>
using Const = std::integral_constant<int, V>;
template <class F>
inline int flag(int v, F&& f) { return v ? f(Const<1>{}) : f(Const<0>{}); }
template <int W>
NT_HD NT_INLINE void item_wcomb_digits(size_t i, const uint32_t* x8, uint32_t* out, Const<W>) {
  item_wcomb_digits<W>(i, x8, out);
}

}  // namespace ntp
