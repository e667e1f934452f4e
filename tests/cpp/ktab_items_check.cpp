// ktab_items_check.cpp -- TEST INFRASTRUCTURE: a stand-alone driver of the probe's
// key-table items (nt_probe_items.hpp: item_ktab_fill, item_ktab_point) over
// HostKTab (ktab/host_ktab.hpp) for host sanitizer runs:
//   make -C tests/cpp build/ktab_items_check && tests/cpp/build/ktab_items_check
// (g++ -fsanitize=address,undefined -fno-sanitize-recover=all).
// The table is one heap allocation of exactly ntp::ktab_probe_bytes(capacity)
// bytes -- control block, index, pool, as the device probe lays it out -- so a
// slot, header or point address past either end is reported.  Keys: encodings
// y = 2, 3, ... (about half decode), the small-order y = 0, 1 and p - 1, one key
// five times; first with room for every key, then with a pool of 4.  What it
// checks besides the addresses is what needs no curve model: entries handed
// out, tags, flags, digit 0 = the identity, digit 1 of table 0 = the key, and
// digit -d = the negative of digit d.  Exit status 0 = clean.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nt_probe_items.hpp"
#include "ktab/host_ktab.hpp"

using namespace nt;

static int fails = 0;
#define EXPECT(c)                                               \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("line %d: %s\n", __LINE__, #c);               \
      ++fails;                                                  \
    }                                                           \
  } while (0)

static int run(const std::vector<uint32_t>& keys, uint32_t capacity, uint32_t distinct) {
  const uint64_t n = keys.size() / 8;
  const size_t bytes = ntp::ktab_probe_bytes(capacity);
  uint8_t* blob = (uint8_t*)std::calloc(bytes, 1);
  if (!blob) return 1;
  const HostKTab kt{(uint64_t*)(blob + ntp::kKtProbeCtlBytes), ntp::kKtProbeSlots - 1u, blob + ntp::kKtProbePoolOff,
                    capacity, (uint32_t*)blob};
  std::vector<uint32_t> slot(n);
  for (uint64_t i = 0; i < n; ++i) ntp::item_ktab_fill(i, keys.data(), kt, slot.data(), true);
  const uint32_t want_used = distinct < capacity ? distinct : capacity;
  EXPECT(kt.pool_used() == want_used);
  uint32_t won = 0;
  for (uint64_t i = 0; i < n; ++i) won += slot[i] != kKtNoSlot;
  EXPECT(won == want_used);
  // every (key, table, digit)
  std::vector<uint32_t> A;
  std::vector<int32_t> td;
  for (uint64_t i = 0; i < n; ++i)
    for (int t = 0; t < 3; ++t)
      for (int d = -8; d <= 8; ++d) {
        A.insert(A.end(), keys.begin() + 8 * i, keys.begin() + 8 * i + 8);
        td.push_back(t);
        td.push_back(d);
      }
  const uint64_t m = td.size() / 2;
  std::vector<uint32_t> out3(3 * m), enc(8 * m);
  for (uint64_t j = 0; j < m; ++j) ntp::item_ktab_point(j, A.data(), td.data(), kt, out3.data(), enc.data());
  uint32_t ready = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t j0 = i * 51;
    const uint32_t idx = out3[3 * j0];
    if (idx == kKtNoSlot) continue;
    ++ready;
    EXPECT(idx < capacity);
    EXPECT(out3[3 * j0 + 1] == 1u);
    ge_p3 P;
    const uint32_t ok = ge_frombytes_w(P, keys.data() + 8 * i);
    const uint32_t flags = out3[3 * j0 + 2];
    EXPECT(((flags & kKtUndecodable) != 0) == (ok == 0));
    if (!ok) continue;
    EXPECT(((flags & kKtSmallOrder) != 0) == (ge_is_small_order(P) != 0));
    for (int t = 0; t < 3; ++t) {
      const uint32_t* e = enc.data() + 8 * (j0 + 17 * t);  // digits -8 .. 8
      const uint32_t* zero = e + 8 * 8;
      EXPECT(zero[0] == 1u);
      for (int l = 1; l < 8; ++l) EXPECT(zero[l] == 0u);
      for (int d = 1; d <= 8; ++d) {
        const uint32_t *pos = e + 8 * (8 + d), *neg = e + 8 * (8 - d);
        for (int l = 0; l < 7; ++l) EXPECT(pos[l] == neg[l]);
        EXPECT((pos[7] & 0x7fffffffu) == (neg[7] & 0x7fffffffu));
      }
      if (t == 0) {  // digit 1 of table 0 is the key itself (these keys are canonical encodings)
        uint32_t y[8], x[8];
        fe_tobytes_w(y, P.Y);
        fe_tobytes_w(x, P.X);
        y[7] |= (x[0] & 1u) << 31;
        EXPECT(std::memcmp(e + 8 * 9, y, 32) == 0);
      }
    }
  }
  if (distinct <= capacity) EXPECT(ready == n);
  else EXPECT(ready >= capacity);  // a key on several lanes counts once per lane
  std::free(blob);
  return 0;
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
  if (fails) {
    std::printf("ktab_items_check: %d failures\n", fails);
    return 1;
  }
  std::printf("ktab_items_check: %zu keys, capacities 64 and 4: clean\n", keys.size() / 8);
  return 0;
}
