// kcomb_items_check.cpp -- TEST INFRASTRUCTURE: a stand-alone driver of the probe's comb items of
// the key-table cache (nt_probe_items.hpp: item_kcomb_fill, item_kcomb_line, item_kc_picks,
// item_ladder_kc, item_compare_one, item_verify_kc) over HostKComb (kcomb/host_kcomb.hpp) for host
// sanitizer runs:
//   make -C tests/cpp build/kcomb_items_check && tests/cpp/build/kcomb_items_check
// (g++ -fsanitize=address,undefined -fno-sanitize-recover=all).
// The table is one heap allocation of exactly ntp::kcomb_probe_bytes(capacity) bytes -- control
// block, index, pool, comb pool, guard, as the device probe lays it out -- so a slot, header or
// line address past either end is reported.  Keys: those of ktab_items_check (encodings y = 2,
// 3, ...: about half decode; the small-order y = 0, 1 and p - 1; one key five times), first with
// room for every key, then with a pool of 4.  What it checks besides the addresses is what needs
// no curve model: entries handed out, tags, flags, line 32 = the key's affine niels form, a line
// number past 32 = line 32, prefill kept where nothing is stored, picks in range, a dead lane's
// identity, [1](-A) and [2](-A) against the header's own arithmetic, compare_one and verify_kc on
// the identity.  Exit status 0 = clean.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nt_probe_items.hpp"
#include "kcomb/host_kcomb.hpp"

using namespace nt;

static int fails = 0;
#define EXPECT(c)                                               \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("line %d: %s\n", __LINE__, #c);               \
      ++fails;                                                  \
    }                                                           \
  } while (0)

namespace {
struct HostATab {
  ge_cached e[18];
  void store(uint32_t j, const ge_cached& c) { e[j] = c; }
  void load(uint32_t j, ge_cached& c) const { c = e[j]; }
  void load_signed(uint32_t e0, int32_t d, ge_cached& c) const {
    c = e[e0 + (uint32_t)(d < 0 ? -d : d)];
    ge_cached_cneg(c, d < 0);
  }
};
// the comb of B the verdict item needs: every entry by double-and-add (16-bit digits)
struct SlowBComb {
  static constexpr int kBits = kKeyCombNarrow;
  ge_p3 B;
  void load(uint32_t pos, uint32_t idx, ge_niels& q) const {
    ge_p3 base = B;
    for (uint32_t r = 0; r < pos * (uint32_t)kBits; ++r) {
      ge_p2 t2;
      ge_p3_to_p2(t2, base);
      ge_cp t;
      ge_dbl(t, t2);
      ge_cp_to_p3(base, t);
    }
    ge_cached Pc;
    ge_p3_to_cached(Pc, base);
    ge_p3 Q;
    ge_p3_0(Q);
    for (int bit = kBits - 1; bit >= 0; --bit) {
      ge_p2 q2;
      ge_p3_to_p2(q2, Q);
      ge_cp t;
      ge_dbl(t, q2);
      ge_cp_to_p3(Q, t);
      if ((idx >> bit) & 1u) {
        ge_add_cached(t, Q, Pc);
        ge_cp_to_p3(Q, t);
      }
    }
    fe zi;
    fe_invert(zi, Q.Z);
    ge_niels_from(q, Q.X, Q.Y, zi);
  }
  void load_corr(ge_niels& q) const { ge_niels_0(q); }
};
constexpr uint8_t kFill = 0xA5;

HostKComb blob_kcomb(uint8_t* blob, uint32_t capacity) {
  return HostKComb((uint64_t*)(blob + ntp::kKtProbeCtlBytes), ntp::kKtProbeSlots - 1u, blob + ntp::kKtProbePoolOff, capacity,
                   (uint32_t*)blob, blob + ntp::kcomb_probe_comb_off(capacity));
}
bool all_fill(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (p[i] != kFill) return false;
  return true;
}
void encode(uint32_t out[8], const ge_p3& P) {
  ge_p2 p;
  ge_p3_to_p2(p, P);
  ge_tobytes_w(out, p);
}
}  // namespace

static int run(const std::vector<uint32_t>& keys, uint32_t capacity, uint32_t distinct) {
  const uint64_t n = keys.size() / 8;
  const size_t bytes = ntp::kcomb_probe_bytes(capacity);
  uint8_t* blob = (uint8_t*)std::malloc(bytes);
  if (!blob) return 1;
  std::memset(blob, kFill, bytes);
  std::memset(blob, 0, ntp::kKtProbePoolOff);
  const HostKComb kt = blob_kcomb(blob, capacity);
  EXPECT(kt.has_comb());
  std::vector<uint32_t> slot(n);
  for (uint64_t i = 0; i < n; ++i) {
    HostATab at;
    ntp::item_kcomb_fill(i, keys.data(), kt, at, slot.data(), true);
  }
  const uint32_t want_used = distinct < capacity ? distinct : capacity;
  uint32_t won = 0;
  for (uint64_t i = 0; i < n; ++i) won += slot[i] != kKtNoSlot;
  EXPECT(won >= want_used && kt.pool_used() == won);
  // every (key, line 0 .. 32) and three numbers past the last line
  const uint32_t extra[3] = {kKcEntries, 40u, 0xffffffffu};
  const uint32_t per = kKcEntries + 3;
  std::vector<uint32_t> A, line;
  for (uint64_t i = 0; i < n; ++i)
    for (uint32_t l = 0; l < per; ++l) {
      A.insert(A.end(), keys.begin() + 8 * i, keys.begin() + 8 * i + 8);
      line.push_back(l < kKcEntries ? l : extra[l - kKcEntries]);
    }
  const uint64_t m = line.size();
  std::vector<uint32_t> out3(3 * m), limbs(30 * m);
  for (uint64_t j = 0; j < m; ++j) ntp::item_kcomb_line(j, A.data(), line.data(), kt, out3.data(), limbs.data());
  uint32_t ready = 0;
  std::vector<uint32_t> kidx, k8, dead, live_key;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t j0 = i * per;
    const uint32_t idx = out3[3 * j0];
    if (idx == kKtNoSlot) continue;
    ++ready;
    EXPECT(idx < capacity);
    EXPECT(out3[3 * j0 + 1] == 1u);
    ge_p3 P;
    const uint32_t ok = ge_frombytes_w(P, keys.data() + 8 * i);
    const uint32_t flags = out3[3 * j0 + 2];
    EXPECT(((flags & kKtUndecodable) != 0) == (ok == 0));
    const uint8_t* comb = blob + ntp::kcomb_probe_comb_off(capacity) + (size_t)idx * kKtCombBytes;
    const uint8_t* entry = blob + ntp::kKtProbePoolOff + (size_t)idx * kKtEntryBytes;
    EXPECT(all_fill(entry + kKtHeaderBytes, kKtEntryBytes - kKtHeaderBytes));
    if (!ok) {
      EXPECT(all_fill(comb, kKtCombBytes));
      continue;
    }
    EXPECT(((flags & kKtSmallOrder) != 0) == (ge_is_small_order(P) != 0));
    for (uint32_t l = 0; l < kKcEntries; ++l) {
      EXPECT(all_fill(comb + l * kKcLineBytes + 120, 8));
      EXPECT(std::memcmp(comb + l * kKcLineBytes, limbs.data() + 30 * (j0 + l), 120) == 0);
    }
    for (uint32_t l = kKcEntries; l < per; ++l)  // the clamp: line 32
      EXPECT(std::memcmp(limbs.data() + 30 * (j0 + l), limbs.data() + 30 * (j0 + kKcSigned), 120) == 0);
    {  // line 32 is the key: (y + x, y - x, 2 d x y) of the decoded point (Z = 1)
      fe one;
      fe_1(one);
      ge_niels q;
      ge_niels_from(q, P.X, P.Y, one);
      const uint32_t* w = limbs.data() + 30 * (j0 + kKcSigned);
      fe a, b, c;
      for (int t = 0; t < 10; ++t) { a.v[t] = w[t]; b.v[t] = w[10 + t]; c.v[t] = w[20 + t]; }
      EXPECT(fe_eq(a, q.ypx) && fe_eq(b, q.ymx) && fe_eq(c, q.xy2d));
    }
    // the ladder on this entry: k = 0, 1, 2, 2^64 - 1, 2^253 - 1, live and dead
    const uint32_t ks[5][8] = {{0}, {1}, {2}, {0xffffffffu, 0xffffffffu},
                               {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x1fffffffu}};
    for (int t = 0; t < 5; ++t)
      for (uint32_t d = 0; d < 2; ++d) {
        kidx.push_back(idx);
        dead.push_back(d);
        k8.insert(k8.end(), ks[t], ks[t] + 8);
        live_key.push_back((uint32_t)i);
      }
  }
  if (distinct <= capacity) EXPECT(ready == n);
  else EXPECT(ready >= capacity);  // a key on several lanes counts once per lane
  // nothing behind the entries and combs handed out, and the guard
  const uint32_t used = kt.pool_used() < capacity ? kt.pool_used() : capacity;
  EXPECT(all_fill(blob + ntp::kKtProbePoolOff + (size_t)used * kKtEntryBytes, (size_t)(capacity - used) * kKtEntryBytes));
  EXPECT(all_fill(blob + ntp::kcomb_probe_comb_off(capacity) + (size_t)used * kKtCombBytes,
                  (size_t)(capacity - used) * kKtCombBytes + ntp::kKcProbeGuardBytes));
  // the ladder
  const uint64_t nl = kidx.size();
  EXPECT(ntp::ladder_kc_args_ok(nl, kidx.data(), k8.data(), dead.data(), capacity));
  std::vector<uint32_t> enc(8 * nl);
  for (uint64_t j = 0; j < nl; ++j) ntp::item_ladder_kc(j, kidx.data(), k8.data(), dead.data(), kt, enc.data(), true);
  for (uint64_t j = 0; j < nl; ++j) {
    const uint32_t* e = enc.data() + 8 * j;
    const int t = (int)(j / 2 % 5);
    uint32_t want[8] = {1, 0, 0, 0, 0, 0, 0, 0};  // the identity: dead lanes and k = 0
    if (!dead[j] && (t == 1 || t == 2)) {
      ge_p3 P, Q;
      ge_frombytes_w(P, keys.data() + 8 * live_key[j]);
      fe_neg(P.X, P.X);
      fe_carry(P.X);
      fe_neg(P.T, P.T);
      fe_carry(P.T);
      Q = P;
      if (t == 2) {
        ge_p2 p2;
        ge_p3_to_p2(p2, P);
        ge_cp c;
        ge_dbl(c, p2);
        ge_cp_to_p3(Q, c);
      }
      encode(want, Q);
    }
    if (dead[j] || t <= 2) EXPECT(std::memcmp(e, want, 32) == 0);
  }
  std::free(blob);
  return 0;
}

static void picks_compare_verify() {
  // picks: in range, block i mod 4, c the parity's complement
  const uint32_t ks[4][8] = {{0}, {1}, {0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x1fffffffu},
                             {0x00010001u, 0x00010000u, 1u, 0xffff0000u, 0x0000ffffu, 0x80000000u, 0x7fffffffu, 0x10000000u}};
  uint64_t slots[kKtBucket] = {};
  uint32_t ctl[4] = {};
  const HostKComb kd(slots, kKtBucket - 1, nullptr, 0, ctl, nullptr);
  EXPECT(ntp::kc_scalars_ok(4, &ks[0][0]));
  std::vector<uint32_t> out(4 * ntp::kKcPickWords);
  for (size_t i = 0; i < 4; ++i) ntp::item_kc_picks(i, &ks[0][0], kd, out.data());
  for (size_t i = 0; i < 4; ++i) {
    const uint32_t* o = out.data() + ntp::kKcPickWords * i;
    for (uint32_t t = 0; t < 64; ++t) EXPECT((o[t] & 0xffu) / kKcPerBlock == t % 4 && (o[t] >> 8) <= 1u);
    EXPECT(o[64] == ((ks[i][0] & 1u) ^ 1u));
  }
  const uint32_t bad[8] = {0, 0, 0, 0, 0, 0, 0, 0x20000000u};
  EXPECT(!ntp::kc_scalars_ok(1, bad));
  // compare_one: the identity (0 : z : z) against its encoding, both modes, and against y = 2
  const uint32_t zero[8] = {0}, one[8] = {1}, z[8] = {12345, 6789, 1, 2, 3, 4, 5, 6}, two[8] = {2};
  const uint32_t x3[24] = {0}, y3[24] = {1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1};
  uint32_t z3[24], R3[24], mode3[3] = {0, 1, 1}, bit[3];
  for (int i = 0; i < 3; ++i) {
    std::memcpy(z3 + 8 * i, z, 32);
    std::memcpy(R3 + 8 * i, i == 2 ? two : one, 32);
  }
  (void)zero;
  EXPECT(ntp::modes_ok(3, mode3));
  for (size_t i = 0; i < 3; ++i) ntp::item_compare_one(i, x3, y3, z3, R3, mode3, bit);
  EXPECT(bit[0] == 0u && bit[1] == 1u && bit[2] == 0u);  // strict: small order; cofactorless: equal; y differs
  // verify_kc with s = 0, k = 0 over a dead entry index 0 of a one-entry table nothing was built in:
  // R' is the identity whatever the comb holds -- flags 0: cofactorless accepts the identity's
  // encoding, strict rejects; flags undecodable: rejected
  const size_t bytes = ntp::kcomb_probe_bytes(1);
  uint8_t* blob = (uint8_t*)std::malloc(bytes);
  if (!blob) { ++fails; return; }
  std::memset(blob, kFill, bytes);
  std::memset(blob, 0, ntp::kKtProbePoolOff);
  const HostKComb kt = blob_kcomb(blob, 1);
  {  // the comb of key y = 3 (decodes) in entry 0
    const uint32_t key[8] = {3};
    uint32_t slot[1];
    HostATab at;
    ntp::item_kcomb_fill(0, key, kt, at, slot, true);
    EXPECT(slot[0] != kKtNoSlot && kt.pool_used() == 1u);
  }
  SlowBComb wb;
  {
    uint32_t enc[8];
    for (int i = 0; i < 8; ++i) enc[i] = kBaseEnc[i];
    EXPECT(ge_frombytes_w(wb.B, enc));
  }
  const uint32_t kidx[3] = {0, 0, 0}, kflags[3] = {0, 0, kKtUndecodable}, vm[3] = {0, 1, 1};
  uint32_t R[24], S[24] = {0}, K[24] = {0}, ok[3];
  for (int i = 0; i < 3; ++i) std::memcpy(R + 8 * i, one, 32);
  EXPECT(ntp::verify_kc_args_ok(3, kidx, kflags, K, vm, 1));
  EXPECT(!ntp::verify_kc_args_ok(3, kidx, kflags, K, vm, 0));
  for (size_t i = 0; i < 3; ++i) ntp::item_verify_kc(i, kidx, kflags, R, S, K, vm, wb, kt, ok, true);
  EXPECT(ok[0] == 0u && ok[1] == 1u && ok[2] == 0u);
  std::free(blob);
}

int main() {
  std::vector<uint32_t> keys;
  uint32_t distinct = 0;
  auto push = [&](uint32_t y0, uint32_t top) {
    uint32_t w[8] = {y0, 0, 0, 0, 0, 0, 0, top};
    keys.insert(keys.end(), w, w + 8);
  };
  for (uint32_t y = 0; y < 40; ++y, ++distinct) push(y, 0);
  for (uint32_t y = 2; y < 12; ++y, ++distinct) push(y, 0x80000000u);  // the other sign of x
  {  // p - 1: the point of order 2
    uint32_t w[8] = {0xffffffecu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu};
    keys.insert(keys.end(), w, w + 8);
    ++distinct;
  }
  for (int r = 0; r < 4; ++r) push(3, 0);  // y = 3 four more times
  if (run(keys, 64, distinct)) return 2;
  if (run(keys, 4, distinct)) return 2;
  picks_compare_verify();
  if (fails) {
    std::printf("kcomb_items_check: %d failures\n", fails);
    return 1;
  }
  std::printf("kcomb_items_check: %zu keys, capacities 64 and 4: clean\n", keys.size() / 8);
  return 0;
}
