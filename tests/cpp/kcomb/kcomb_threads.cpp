// kcomb_threads.cpp -- TEST INFRASTRUCTURE: the key-table cache's claim / build / publish /
// probe code with a comb pool (ktab.hpp ktab_probe, ktab_sight; ktab_build -> ktab_comb.hpp ktab_build_comb)
// and the cached check over it (verify_kc), run by several host threads at once over one index, one
// pool and one comb pool, with host atomics (host_kcomb.hpp).  Every thread walks the same keys in
// its own order; whenever a key's slot reads ready, the entry's tag and all 33 comb lines must be
// the ones a single-threaded build gives, and verify_kc must accept the R' the single-threaded
// entry gives for s = 0 and a fixed k and reject it with one bit flipped (s = 0: the comb of B
// is then only ever asked for its identity entries, which the stand-in below hands out; this
// program includes nothing of the host harness, whose operation counters are plain globals).
// The pool is smaller than the key set, so exhaustion happens under contention as well.  Meant to
// be built with -fsanitize=thread (a data race between a builder's plain stores -- the lines are written twice,
// projective then affine -- and a reader's plain loads is then reported); exit status 0 = consistent.
#include <cstdio>
#include <thread>
#include <vector>

#include "host_kcomb.hpp"

using namespace nt;

namespace {
constexpr uint32_t kKeys = 20, kThreads = 8, kRounds = 3, kSlots = 32, kCap = 16;

uint64_t checksum(const HostKComb& kt, uint32_t idx) {
  uint64_t h = 1469598103934665603ull;
  for (uint32_t e = 0; e < kKcEntries; ++e) {
    ge_niels q;
    kt.comb_load(idx, e, q);
    for (int i = 0; i < 10; ++i) {
      h = (h ^ q.ypx.v[i]) * 1099511628211ull;
      h = (h ^ q.ymx.v[i]) * 1099511628211ull;
      h = (h ^ q.xy2d.v[i]) * 1099511628211ull;
    }
  }
  return h;
}

// the lane's table workspace
struct ATab {
  static constexpr uint32_t kEntries = 18;
  ge_cached e[kEntries];
  void store(uint32_t j, const ge_cached& c) { e[j] = c; }
  void load(uint32_t j, ge_cached& c) const { c = e[j]; }
};
// the comb of B for s = 0: every digit is zero and every entry the identity
struct ZeroBComb {
  static constexpr int kBits = kBCombBits;
  mutable uint32_t nonzero = 0;
  void load(uint32_t, uint32_t idx, ge_niels& q) const {
    nonzero |= idx;
    ge_niels_0(q);
  }
};

struct Key {
  uint32_t w[8];
  uint32_t flags;
  uint64_t sum;
  uint32_t k[8], R[8];  // a scalar below L and the encoding of [s]B - [k]A
};
}  // namespace

int main() {
  uint32_t s[8] = {};
  std::vector<Key> keys(kKeys);
  uint64_t x = 0x243f6a8885a308d3ull;
  {
    const ZeroBComb wb;
    for (Key& k : keys) {
      // keys: xorshift bytes (about half of them decode)
      for (int i = 0; i < 8; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        k.w[i] = (uint32_t)(x >> 16);
        k.k[i] = (uint32_t)(x >> 8);
      }
      k.k[7] &= 0x0fffffffu;  // < 2^252 < L
      k.k[0] = (k.k[0] & ~1u) | (uint32_t)((&k - keys.data()) & 1);  // both parities
      // the reference: a single-threaded build into a private entry
      uint64_t slots[kKtBucket] = {};
      std::vector<uint8_t> pool(kKtEntryBytes, 0), comb(kKtCombBytes, 0);
      uint32_t ctl[4] = {};
      const HostKComb kt(slots, kKtBucket - 1, pool.data(), 1, ctl, comb.data());
      ATab at;
      ktab_build(k.w, 0u, kt, at);
      if (slots[0] != ktab_word(ktab_fp(k.w), kKtReady0)) return 2;
      uint32_t tag[8];
      kt.hdr_load(0, tag, k.flags);
      k.sum = checksum(kt, 0);
      ge_cp t;
      ladder_kc(t, k.k, (k.flags & kKtUndecodable) ? 1u : 0u, kt, 0u);
      ge_p3 acc;
      ge_cp_to_p3(acc, t);
      wcomb_acc(acc, s, wb);
      ge_p2 P;
      ge_p3_to_p2(P, acc);
      ge_tobytes_w(k.R, P);
    }
  }
  unsigned decodable = 0;
  for (const Key& k : keys) decodable += (k.flags & kKtUndecodable) ? 0u : 1u;

  std::vector<uint64_t> slots(kSlots, 0);
  std::vector<uint8_t> pool((size_t)kCap * kKtEntryBytes, 0), comb((size_t)kCap * kKtCombBytes, 0);
  uint32_t ctl[4] = {};
  uint32_t bad = 0, hits = 0, builds = 0;
  std::vector<std::thread> th;
  for (uint32_t t = 0; t < kThreads; ++t)
    th.emplace_back([&, t] {
      // the policy carries the digit words of the verification in flight: one per thread
      const HostKComb kt(slots.data(), kSlots - 1, pool.data(), kCap, ctl, comb.data());
      const ZeroBComb wb;
      ATab at;
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
            if (flags & kKtUndecodable) continue;
            if (checksum(kt, idx) != k.sum) ++mybad;
            uint32_t R[8];
            std::memcpy(R, k.R, 32);
            if (verify_kc<kCofactorless>(R, s, k.k, flags, wb, kt, idx) != 1u) ++mybad;
            R[3] ^= 0x400u;
            if (verify_kc<kCofactorless>(R, s, k.k, flags, wb, kt, idx) != 0u) ++mybad;
          } else if (ktab_sight(p, kt)) {
            ++mybuilds;
            ktab_build(k.w, p.slot, kt, at);
          }
        }
      if (wb.nonzero) ++mybad;
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
