// wcomb_build_check.cpp -- TEST INFRASTRUCTURE: a stand-alone driver of the wide-comb
// construction (wcomb_build.hpp: wcomb_key_bases, wcomb_fill_launch, wcomb_fill_target;
// ed25519_ops.hpp: wcomb_fill) and of the probe's comb items (nt_probe_items.hpp) for host
// sanitizer runs:
//   make -C tests/cpp build/wcomb_build_check && tests/cpp/build/wcomb_build_check
// (g++ -fsanitize=address,undefined -fno-sanitize-recover=all).
// It builds the 16-bit combs of three keys, two per fill batch, as wcomb_build<16> launches
// them -- every thread of each launch's grid -- into heap allocations of exactly the sizes the
// product allocates (combs, bases, tmp for one batch), so a destination or scratch address
// past either end is reported.  What it checks besides the addresses needs no curve model:
// no word of a comb is left unwritten, words 30 and 31 of every entry are zero, entry 0 is the
// identity, [1]P from the table is the key, [x]P + [-x]P is the identity, and the loads
// wcomb_acc issues are the digits of the schedule.  Exit status 0 = clean.
#include <cstdio>
#include <cstring>
#include <vector>

#include "nt_probe_items.hpp"

using namespace nt;

static int fails = 0;
#define EXPECT(c)                                 \
  do {                                            \
    if (!(c)) {                                   \
      if (fails < 20) std::printf("line %d: %s\n", __LINE__, #c); \
      ++fails;                                    \
    }                                             \
  } while (0)

constexpr int W = kKeyCombNarrow;
using G = CombGeom<W>;
struct TabComb {  // a built comb in memory, read as WideComb<W> reads it
  static constexpr int kBits = W;
  const uint32_t* base;
  void load(uint32_t pos, uint32_t idx, ge_niels& q) const {
    const uint32_t* e = base + ((size_t)pos * G::kEntries + idx) * kWStride;
    for (int l = 0; l < 10; ++l) { q.ypx.v[l] = e[l]; q.ymx.v[l] = e[10 + l]; q.xy2d.v[l] = e[20 + l]; }
  }
  void load_corr(ge_niels& q) const { ge_niels_0(q); }
};

int main() {
  const uint32_t nkeys = 3, batch = 2, kFill = 0xA5A5A5A5u;
  uint32_t enc[8 * nkeys] = {};
  for (int i = 0; i < 8; ++i) enc[i] = kBaseEnc[i];
  enc[8] = 3;   // y = 3 decodes
  enc[16] = 2;  // y = 2 does not
  std::vector<uint32_t> comb((size_t)nkeys * G::kWordsPerPoint, kFill), bases(comb_size<W>(1) / 4 * nkeys),
      tmp(comb_size<W>(2) / 4 * batch), corr(kWStride);
  uint32_t meta[nkeys];
  for (uint32_t k = 0; k < nkeys; ++k)
    wcomb_key_bases<W>(enc + 8 * k, k == 1, bases.data() + (size_t)k * G::kPos * 40, corr.data(), meta + k);
  EXPECT(meta[0] == kKeyDecodes && meta[1] == kKeyDecodes && !(meta[2] & kKeyDecodes));
  uint32_t launches = 0;
  for (uint32_t k0 = 0; k0 < nkeys; k0 += batch, ++launches) {
    const WCombFillLaunch fl = wcomb_fill_launch<W>(k0, nkeys, batch);
    for (uint64_t t = 0; t < (fl.threads + 63) / 64 * 64; ++t) {
      WCombFillTarget ft;
      if (!wcomb_fill_target<W>(ft, t, fl.nkeys)) continue;
      wcomb_fill<W>(comb.data() + fl.comb_off + ft.dst, tmp.data() + ft.tmp,
                    bases.data() + fl.bases_off + ((size_t)ft.key * G::kPos + ft.pos) * 40, ft.chunk);
    }
  }
  EXPECT(launches == 2);
  ge_niels id;
  ge_niels_0(id);
  for (uint32_t k = 0; k < nkeys; ++k)
    for (int pos = 0; pos < G::kPos; ++pos)
      for (int idx = 0; idx < G::kEntries; ++idx) {
        const uint32_t* e = comb.data() + (size_t)k * G::kWordsPerPoint + ((size_t)pos * G::kEntries + idx) * kWStride;
        bool unwritten = false;
        for (int l = 0; l < 30; ++l) unwritten |= e[l] == kFill;
        EXPECT(!unwritten);
        EXPECT(e[30] == 0 && e[31] == 0);
        if (idx == 0)  // (the undecodable key's other entries are the identity with unreduced limbs: see the sums)
          for (int l = 0; l < 10; ++l) EXPECT(e[l] == id.ypx.v[l] && e[10 + l] == id.ymx.v[l] && e[20 + l] == id.xy2d.v[l]);
      }
  // sums over the tables: x, flags 1 (from the identity), 3 (negated), then the second added to the first
  const uint32_t xs[4][8] = {{1, 0, 0, 0, 0, 0, 0, 0},
                             {0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u, 0x8000u},
                             {0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x1fffffffu},
                             {0x12345678u, 0x9abcdef0u, 0x0fedcba9u, 0x87654321u, 0xdeadbeefu, 0x01234567u, 0x89abcdefu, 0x0fffffffu}};
  const uint32_t ident[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t k = 0; k < nkeys; ++k) {
    const TabComb wc{comb.data() + (size_t)k * G::kWordsPerPoint};
    for (int j = 0; j < 4; ++j) {
      EXPECT(ntp::wcomb_scalar_ok<W>(xs[j]));
      uint32_t x2[16], fl[2] = {1, 3}, st[16] = {}, out[16];
      std::memcpy(x2, xs[j], 32);
      std::memcpy(x2 + 8, xs[j], 32);
      ntp::item_wcomb_acc(0, wc, x2, fl, st, out);
      ntp::item_wcomb_acc(1, wc, x2, fl, st, out);
      if (j == 0 && k == 0) EXPECT(std::memcmp(out, kBaseEnc, 32) == 0);  // [1]B
      if (k == 2) EXPECT(std::memcmp(out, ident, 32) == 0);               // the undecodable key's comb
      uint32_t fl2[2] = {0, 0}, sum[16];
      std::memcpy(st + 8, out + 8, 32);  // start = [-x]P
      ntp::item_wcomb_acc(1, wc, x2, fl2, st, sum);
      EXPECT(std::memcmp(sum + 8, ident, 32) == 0);
      uint32_t e32[32];
      ntp::item_wcomb_entry(0, TabComb{comb.data()}, (uint32_t)G::kPos - 1, (uint32_t)G::kEntries - 1, e32);
      EXPECT(e32[30] == 0 && e32[31] == 0);
    }
  }
  for (int j = 0; j < 4; ++j) {
    uint32_t out[ntp::kWcDigitWords];
    ntp::item_wcomb_digits<W>(0, xs[j], out);
    EXPECT(out[17] == (uint32_t)G::kPos + 1);
    for (int p = 0; p <= G::kPos; ++p) {
      const int32_t d = (int32_t)out[p];
      EXPECT(out[18 + 2 * p] == (uint32_t)(p < G::kPos ? p : G::kPos - 1) && out[19 + 2 * p] == (uint32_t)(d < 0 ? -d : d));
    }
  }
  if (fails) {
    std::printf("wcomb_build_check: %d failures\n", fails);
    return 1;
  }
  std::printf("wcomb_build_check: %u keys at %d bits, %u fill launches: clean\n", nkeys, W, launches);
  return 0;
}
