// TEST INFRASTRUCTURE: the worker's layout walk (narwhal-tusk_amd/csrc/
// wmsg_plan.hpp) compiled for the host -- the W = 64 speculation in a loop, the
// rounds the device runs -- behind a loader that refuses every read outside the
// message.
//   libnthost_wmsgplan.so  ntwm_walk() for tests/test_wmsg_plan.py (ctypes): the
//                          64-byte receipt of one message (digest: a request's
//                          key; a batch's left zero), whether a read fell outside,
//                          and the rounds the batch walk took
//   wmsg_plan_check        (-DNT_WMSGPLAN_MAIN, built with -fsanitize=address,
//                          undefined) a stand-alone program: builds batches and
//                          requests, mutates them (flips, count and prefix
//                          overwrites up to 2^64 - 1 and values that would wrap,
//                          truncation at every byte of small messages, splices,
//                          trailing bytes, garbage), copies each into a heap block
//                          of exactly its length and walks it; an out-of-range
//                          read aborts, and so does a plan that differs from a
//                          serial decoder written out below
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../../narwhal-tusk_amd/csrc/wmsg_plan.hpp"

namespace {

struct CheckedLd {
  const uint8_t* p;
  uint64_t n;
  bool* oob;
  bool in(uint64_t o, uint64_t k) const {
    if (o <= n && n - o >= k) return true;
    *oob = true;
#ifdef NT_WMSGPLAN_MAIN
    fprintf(stderr, "wmsg_plan: read of %llu bytes at %llu outside a message of %llu\n", (unsigned long long)k,
            (unsigned long long)o, (unsigned long long)n);
    abort();
#endif
    return false;
  }
  uint32_t u8(uint64_t o) const { return in(o, 1) ? p[o] : 0u; }
  uint32_t u32(uint64_t o) const {
    uint32_t x = 0;
    if (in(o, 4)) memcpy(&x, p + o, 4);
    return x;
  }
  uint64_t u64(uint64_t o) const {
    uint64_t x = 0;
    if (in(o, 8)) memcpy(&x, p + o, 8);
    return x;
  }
};

}  // namespace

// rec64: the receipt (nt_worker_receipt) with a batch's digest left zero;
// out[0] = 1 if any read fell outside [0, len), out[1] = rounds of the batch walk
extern "C" void ntwm_walk(const uint8_t* data, uint64_t len, uint8_t* rec64, uint64_t* out) {
  bool oob = false;
  const CheckedLd ld{data, len, &oob};
  uint8_t key[32] = {0};
  uint64_t rounds = 0;
  const nt::WmsgPlan m = nt::wmsg_walk(ld, len, key, &rounds);
  uint32_t dig[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w[nt::kWmsgReceiptWords];
  if (m.code == nt::kWmsgOk && m.kind == nt::kWmsgRequest) memcpy(dig, key, 32);
  nt::wmsg_receipt_words(m, dig, w);
  memcpy(rec64, w, 64);
  out[0] = oob;
  out[1] = rounds;
}

// The lanes whose prefix straddled the end of the message in some round of the batch walk
// (it starts inside [0, len) and ends outside): bit j = lane j.  The rounds are wmsg_walk's,
// from the same pieces; tests use it to show which lane a shape puts on the edge.
extern "C" uint64_t ntwm_straddlers(const uint8_t* data, uint64_t len) {
  bool oob = false;
  const CheckedLd ld{data, len, &oob};
  const nt::WmsgPlan m = nt::wmsg_head(ld, len);
  if (m.code != nt::kWmsgOk || m.kind != nt::kWmsgBatch) return 0;
  nt::WmsgWalk w = nt::wmsg_walk_start(m);
  uint64_t edge = 0;
  while (w.r) {
    uint64_t q[nt::kWmsgLanes], v[nt::kWmsgLanes], agree = 0;
    bool valid[nt::kWmsgLanes];
    for (uint32_t j = 0; j < nt::kWmsgLanes; ++j) {
      valid[j] = nt::wmsg_lane_at(w, len, j, &q[j]);
      v[j] = valid[j] ? ld.u64(q[j]) : 0;
      if (!valid[j] && j < w.r && w.h < len) {  // where the lane would have read (no wrap: h < len < 2^56)
        const uint64_t at = w.p + (uint64_t)j * (8 + w.h);
        if (at < len && len - at < 8) edge |= 1ull << j;
      }
    }
    for (uint32_t j = 0; j < nt::kWmsgLanes; ++j)
      if (nt::wmsg_lane_agrees(w, len, j, valid[j], q[j], v[j], v[0])) agree |= 1ull << j;
    const uint64_t na = ~agree;
    const uint32_t k = na ? (uint32_t)__builtin_ctzll(na) : 0u;
    nt::wmsg_round_end(w, valid[0], v[0], agree, valid[k], v[k]);
  }
  return edge;
}

#ifdef NT_WMSGPLAN_MAIN
namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}
uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

typedef std::vector<uint8_t> Bytes;
void put(Bytes& b, uint64_t x, int n) {
  for (int i = 0; i < n; ++i) b.push_back((uint8_t)(x >> (8 * i)));
}
void fill(Bytes& b, size_t n) {
  for (size_t i = 0; i < n; ++i) b.push_back((uint8_t)rnd());
}
const char kAlphabet[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";

// shape 0: uniform; 1: uniform with one odd transaction; 2: all different; 3: runs of equal lengths;
// 4: data full of the prefix value (coincidences at the speculated positions)
Bytes batch(int shape) {
  Bytes b;
  put(b, 0, 4);
  const uint64_t ntx = below(4) ? below(200) : below(3);
  const uint64_t base = below(3) ? below(40) : below(600);
  const uint64_t odd = below(ntx ? ntx : 1);
  put(b, ntx, 8);
  uint64_t len = base;
  for (uint64_t k = 0; k < ntx; ++k) {
    if (shape == 1) len = k == odd ? base + 1 + below(9) : base;
    if (shape == 2) len = below(70);
    if (shape == 3 && below(20) == 0) len = below(70);
    put(b, len, 8);
    if (shape == 4) {
      for (uint64_t i = 0; i < len; ++i) b.push_back((uint8_t)(i % 8 == 0 ? base : 0));
    } else {
      fill(b, len);
    }
  }
  return b;
}
Bytes request() {
  Bytes b;
  put(b, 1, 4);
  const uint64_t nd = below(6);
  put(b, nd, 8);
  fill(b, 32 * nd);
  put(b, 44, 8);
  for (int i = 0; i < 42; ++i) b.push_back((uint8_t)kAlphabet[below(64)]);
  b.push_back((uint8_t)kAlphabet[4 * below(16)]);  // trailing bits zero
  b.push_back('=');
  return b;
}

// bincode's own order, one transaction at a time: the reference for the speculation
struct Serial {
  uint32_t code = 9, kind = 0xff, uniform = 0;
  uint64_t n = 0, used = 0, tx_bytes = 0, tx_len = 0, off_key = 0;
};
uint64_t rd(const Bytes& m, uint64_t o, int n) {
  uint64_t x = 0;
  for (int i = 0; i < n; ++i) x |= (uint64_t)m[o + i] << (8 * i);
  return x;
}
Serial serial(const Bytes& m) {
  Serial s, fail, host;
  host.code = 0xff;
  const uint64_t L = m.size();
  if (L < 4) return fail;
  const uint64_t tag = rd(m, 0, 4);
  if (tag > 1 || L < 12) return fail;
  const uint64_t cnt = rd(m, 4, 8);
  if (tag == 0) {
    if (cnt > (L - 12) / 8) return fail;
    if (cnt > (1u << 24)) return host;
    uint64_t p = 12, first = 0;
    bool uni = cnt >= 1;
    for (uint64_t k = 0; k < cnt; ++k) {
      if (L - p < 8) return fail;
      const uint64_t len = rd(m, p, 8);
      if (len > L - p - 8) return fail;
      if (k == 0) first = len;
      uni = uni && len == first;
      p += 8 + len;
      s.tx_bytes += len;
    }
    s.code = 0;
    s.kind = 0;
    s.n = cnt;
    s.used = p;
    s.uniform = uni;
    s.tx_len = uni ? first : 0;
    return s;
  }
  if (cnt > (L - 12) / 32) return fail;
  if (cnt > (1u << 20)) return host;
  const uint64_t pos = 12 + 32 * cnt;
  if (L - pos < 8) return fail;
  const uint64_t klen = rd(m, pos, 8);
  if (klen > L - pos - 8) return fail;
  if (klen != 44) return host;
  for (int t = 0; t < 44; ++t) {
    const uint8_t c = m[pos + 8 + t];
    const char* at = c ? strchr(kAlphabet, c) : nullptr;
    if (t == 43 ? c != '=' : !at) return host;
    if (t == 42 && ((at - kAlphabet) & 3)) return host;
  }
  s.code = 0;
  s.kind = 1;
  s.n = cnt;
  s.used = pos + 52;
  s.off_key = pos + 8;
  return s;
}

uint64_t counts[4];  // OK batches, OK requests, serialization, host

void check(const Bytes& m, const char* what, long it) {
  // a heap block of exactly the message's length: AddressSanitizer sees what the loader's check would miss
  uint8_t* blk = (uint8_t*)malloc(m.size() ? m.size() : 1);
  if (!m.empty()) memcpy(blk, m.data(), m.size());
  uint8_t rec[64];
  uint64_t out[2];
  ntwm_walk(blk, m.size(), rec, out);
  free(blk);
  const Serial s = serial(m);
  uint32_t w[16];
  memcpy(w, rec, 64);
  const uint64_t used = w[2] | ((uint64_t)w[3] << 32), txb = w[4] | ((uint64_t)w[5] << 32);
  const bool same = (w[0] & 0xff) == s.code && ((w[0] >> 8) & 0xff) == s.kind && (w[0] >> 16) == s.uniform &&
                    w[1] == s.n && used == s.used && txb == s.tx_bytes && w[6] == s.tx_len && w[7] == s.off_key;
  // each round proves a transaction: no more rounds than transactions (a walk that fails stops early)
  const uint64_t ntx = s.kind == 0 ? s.n : m.size() / 8;
  if (!same || used > m.size() || out[1] > ntx) {
    fprintf(stderr, "wmsg_plan: %s %ld: code %u kind %u flags %u n %u used %llu (serial: %u %u %u %llu %llu), "
            "%llu rounds, %zu bytes\n", what, it, w[0] & 0xff, (w[0] >> 8) & 0xff, w[0] >> 16, w[1],
            (unsigned long long)used, s.code, s.kind, s.uniform, (unsigned long long)s.n, (unsigned long long)s.used,
            (unsigned long long)out[1], m.size());
    abort();
  }
  // a uniform batch takes ntx / 64 rounds (and the one that learns the length)
  if (s.kind == 0 && s.uniform && out[1] > ntx / 64 + 2) {
    fprintf(stderr, "wmsg_plan: %s %ld: %llu rounds for %llu equal transactions\n", what, it,
            (unsigned long long)out[1], (unsigned long long)ntx);
    abort();
  }
  counts[s.code == 0 ? s.kind : s.code == 9 ? 2 : 3]++;
}

}  // namespace

int main() {
  std::vector<Bytes> seeds;
  for (int i = 0; i < 96; ++i) seeds.push_back(i % 4 == 3 ? request() : batch(i % 5));
  // every prefix of small messages
  for (int i = 0; i < 24; ++i) {
    Bytes m = i % 2 ? request() : batch(i % 5);
    if (m.size() > 700) m.resize(700);
    for (size_t cut = 0; cut <= m.size(); ++cut) check(Bytes(m.begin(), m.begin() + cut), "prefix", (long)cut);
  }
  const uint64_t big[] = {0, 1, 43, 44, 45, 63, 64, 65, 1ull << 20, (1ull << 20) + 1, 1ull << 24, (1ull << 24) + 1,
                          1ull << 32, 1ull << 56, 1ull << 61, 1ull << 63, ~0ull, ~0ull - 7, ~0ull - 8, ~0ull - 11,
                          ~0ull - 12, ~0ull / 64, ~0ull / 63, ~0ull / 32, ~0ull / 8};
  const uint64_t nbig = sizeof big / sizeof big[0];
  for (long it = 0; it < 200000; ++it) {
    Bytes m = seeds[below(seeds.size())];
    switch (it % 7) {
      case 0: break;  // as built
      case 1:         // flip bits
        for (uint64_t k = 1 + below(5); k && !m.empty(); --k) m[below(m.size())] ^= (uint8_t)(1u << below(8));
        break;
      case 2: {       // overwrite a count / length region
        const uint64_t p = below(3) ? below(m.size() > 8 ? m.size() - 8 : 1) : 4 + 8 * below(3);
        uint64_t x = below(2) ? big[below(nbig)] : rnd();
        if (below(4) == 0) x = ~0ull - below(m.size() + 64);  // values that wrap when an offset is added
        for (int i = 0; i < 8 && p + i < m.size(); ++i) m[p + i] = (uint8_t)(x >> (8 * i));
        break;
      }
      case 3: m.resize(below(m.size())); break;  // truncate
      case 4: {                                  // splice two messages
        const Bytes& o = seeds[below(seeds.size())];
        m.resize(below(m.size()));
        m.insert(m.end(), o.begin() + below(o.size()), o.end());
        break;
      }
      case 5: fill(m, 1 + below(100)); break;  // trailing bytes
      default:                                 // garbage behind a tag 0..2
        m.clear();
        put(m, below(3), 4);
        fill(m, below(300));
    }
    check(m, "iteration", it);
  }
  printf("wmsg_plan_check: batches %llu requests %llu serialization %llu host %llu\n", (unsigned long long)counts[0],
         (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)counts[3]);
  return counts[0] > 10000 && counts[1] > 5000 && counts[2] > 10000 && counts[3] > 1000 ? 0 : 1;
}
#endif
