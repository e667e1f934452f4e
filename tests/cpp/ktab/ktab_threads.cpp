// ktab_threads.cpp -- TEST INFRASTRUCTURE: the key-table cache's claim / build /
// publish / probe code (ktab.hpp ktab_probe, ktab_sight; ktab_tables.hpp ktab_build) run by
// several host threads at once over one index and one pool, with host atomics
// (host_ktab.hpp).  Every thread walks the same keys in its own order; whenever a
// key's slot reads ready, the entry's tag and all 24 table points must be the
// ones a single-threaded build gives.  The pool is smaller than the key set, so
// exhaustion happens under contention as well.  Meant to be built with
// -fsanitize=thread (a data race between a builder's plain stores and a reader's
// plain loads is then reported); exit status 0 = consistent.
#include <cstdio>
#include <thread>
#include <vector>

#include "host_ktab.hpp"

using namespace nt;

namespace {
constexpr uint32_t kKeys = 48, kThreads = 8, kRounds = 6, kSlots = 64, kCap = 40;

uint64_t checksum(const HostKTab& kt, uint32_t idx) {
  uint64_t h = 1469598103934665603ull;
  for (uint32_t t = 0; t < kKtTables; ++t)
    for (int32_t d = -8; d <= 8; ++d) {
      if (d == 0) continue;
      ge_cached c;
      kt.tab_load_signed(idx, t, d, c);
      for (int i = 0; i < 10; ++i) {
        h = (h ^ c.YpX.v[i]) * 1099511628211ull;
        h = (h ^ c.YmX.v[i]) * 1099511628211ull;
        h = (h ^ c.Z2.v[i]) * 1099511628211ull;
        h = (h ^ c.T2d.v[i]) * 1099511628211ull;
      }
    }
  return h;
}

struct Key {
  uint32_t w[8];
  uint32_t flags;
  uint64_t sum;
};
}  // namespace

int main() {
  // keys: xorshift bytes (about half of them decode)
  std::vector<Key> keys(kKeys);
  uint64_t x = 0x243f6a8885a308d3ull;
  for (Key& k : keys) {
    for (int i = 0; i < 8; ++i) {
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      k.w[i] = (uint32_t)(x >> 16);
    }
    // the reference: a single-threaded build into a private entry
    uint64_t slots[kKtBucket] = {};
    std::vector<uint8_t> pool(kKtEntryBytes, 0);
    uint32_t ctl[4] = {};
    const HostKTab one{slots, kKtBucket - 1, pool.data(), 1, ctl};
    ktab_build(k.w, 0u, one);
    uint32_t tag[8];
    one.hdr_load(0, tag, k.flags);
    k.sum = checksum(one, 0);
  }
  unsigned decodable = 0;
  for (const Key& k : keys) decodable += (k.flags & kKtUndecodable) ? 0u : 1u;

  std::vector<uint64_t> slots(kSlots, 0);
  std::vector<uint8_t> pool((size_t)kCap * kKtEntryBytes, 0);
  uint32_t ctl[4] = {};
  const HostKTab kt{slots.data(), kSlots - 1, pool.data(), kCap, ctl};
  uint32_t bad = 0, hits = 0, builds = 0;
  std::vector<std::thread> th;
  for (uint32_t t = 0; t < kThreads; ++t)
    th.emplace_back([&, t] {
      uint32_t mybad = 0, myhits = 0, mybuilds = 0;
      for (uint32_t r = 0; r < kRounds; ++r)
        for (uint32_t q = 0; q < kKeys; ++q) {
          const Key& k = keys[(q * (2 * t + 1) + r) % kKeys];
          KtProbe p;
          ktab_probe(p, k.w, kt);
          const uint32_t idx = ktab_ready_index(p, kt);
          if (idx != kKtNoSlot) {
            kt.acquire();
            uint32_t tag[8], flags;
            kt.hdr_load(idx, tag, flags);
            if (std::memcmp(tag, k.w, 32) != 0) continue;  // another key's fingerprint: a miss
            ++myhits;
            if (flags != k.flags) ++mybad;
            if (!(flags & kKtUndecodable) && checksum(kt, idx) != k.sum) ++mybad;
          } else if (ktab_sight(p, kt)) {
            ++mybuilds;
            ktab_build(k.w, p.slot, kt);
          }
        }
      __atomic_fetch_add(&bad, mybad, __ATOMIC_RELAXED);
      __atomic_fetch_add(&hits, myhits, __ATOMIC_RELAXED);
      __atomic_fetch_add(&builds, mybuilds, __ATOMIC_RELAXED);
    });
  for (auto& t : th) t.join();
  // afterwards: every ready slot names an entry below the capacity
  uint32_t ready = 0;
  for (uint64_t w : slots) {
    const uint32_t st = (uint32_t)(w >> 32);
    if (st >= kKtReady0) {
      ++ready;
      if (st - kKtReady0 >= kCap) ++bad;
    }
  }
  std::printf("keys %u (decodable %u) threads %u: hits %u builds %u ready %u taken %u bad %u\n", kKeys, decodable,
              kThreads, hits, builds, ready, ctl[0], bad);
  return (bad == 0 && hits > 0 && builds > 0 && ready > 0 && ready <= kCap) ? 0 : 1;
}
