// TEST INFRASTRUCTURE: the device parser's layout walk (narwhal-tusk_amd/csrc/
// msg_plan.hpp) compiled for the host, behind a loader that refuses every read
// outside the message.
//   libnthost_msgplan.so   ntmp_walk() for tests/test_msg_plan.py (ctypes): the
//                          plan of one message, whether every key string is one
//                          of the given texts, and whether a read fell outside
//   msg_plan_check         (-DNT_MSGPLAN_MAIN, built with -fsanitize=address,
//                          undefined) a stand-alone program: builds messages of
//                          all four kinds, mutates them (flips, count overwrites,
//                          truncations, splices, garbage), copies each into a
//                          heap block of exactly its length and walks it; an
//                          out-of-range read aborts, and so does a plan whose
//                          fields reach past the length
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../../narwhal-tusk_amd/csrc/msg_plan.hpp"

namespace {

struct CheckedLd {
  const uint8_t* p;
  uint64_t n;
  bool* oob;
  bool in(uint64_t o, uint64_t k) const {
    if (o <= n && n - o >= k) return true;
    *oob = true;
#ifdef NT_MSGPLAN_MAIN
    fprintf(stderr, "msg_plan: read of %llu bytes at %llu outside a message of %llu\n", (unsigned long long)k,
            (unsigned long long)o, (unsigned long long)n);
    abort();
#endif
    return false;
  }
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

bool known_key(const CheckedLd& ld, uint64_t o, const uint8_t* keys44, uint32_t nkeys) {
  if (!ld.in(o, 44)) return false;
  for (uint32_t k = 0; k < nkeys; ++k)
    if (memcmp(ld.p + o, keys44 + 44 * (size_t)k, 44) == 0) return true;
  return false;
}

// bytes of the message the plan covers
uint64_t extent(const nt::MsgPlan& m) {
  switch (m.kind) {
    case nt::kMsgHeader: return m.off_sig + 64;
    case nt::kMsgVote: return nt::kMsgVoteBytes;
    case nt::kMsgCert: return m.off_votes + 116 * m.nv;
    case nt::kMsgRequest: return m.key0 + 44;
  }
  return 0;
}

}  // namespace

// out[0..11]: kind, round, np, nq, nv, nd, off_par, off_id, off_sig, off_votes, key0, key1;
// out[12] = 1 if the device would decide the layout: the kind is in `kinds` and every key
// string (certificate votes included) is one of the nkeys 44-character texts in keys44;
// out[13] = 1 if any read fell outside [0, len); out[14] = the bytes the plan covers
extern "C" void ntmp_walk(const uint8_t* data, uint64_t len, uint32_t kinds, const uint8_t* keys44, uint32_t nkeys,
                          uint64_t* out) {
  bool oob = false;
  const CheckedLd ld{data, len, &oob};
  const nt::MsgPlan m = nt::msg_walk(ld, len, kinds);
  bool dec = m.kind != nt::kMsgHost;
  if (dec) dec = known_key(ld, m.key0, keys44, nkeys);
  if (dec && m.kind == nt::kMsgVote) dec = known_key(ld, m.key1, keys44, nkeys);
  for (uint64_t v = 0; dec && v < m.nv; ++v) {
    const uint64_t q = nt::msg_cert_vote_key(ld, m, v);
    dec = q != 0 && known_key(ld, q, keys44, nkeys);
  }
  const uint64_t f[15] = {m.kind, m.round, m.np, m.nq, m.nv, m.nd, m.off_par, m.off_id, m.off_sig, m.off_votes,
                          m.key0, m.key1, dec, oob, extent(m)};
  memcpy(out, f, sizeof f);
}

#ifdef NT_MSGPLAN_MAIN
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
void key(Bytes& b, const std::vector<std::string>& keys) {
  const std::string& k = keys[below(keys.size())];
  put(b, 44, 8);
  b.insert(b.end(), k.begin(), k.end());
}
void header_body(Bytes& b, const std::vector<std::string>& keys) {
  key(b, keys);
  put(b, rnd() >> below(64), 8);
  const uint64_t np = below(6), nq = below(80);
  put(b, np, 8);
  fill(b, 36 * np);
  put(b, nq, 8);
  fill(b, 32 * nq);
  fill(b, 96);
}
Bytes message(uint32_t tag, const std::vector<std::string>& keys) {
  Bytes b;
  put(b, tag, 4);
  if (tag == 0) {
    header_body(b, keys);
  } else if (tag == 1) {
    fill(b, 32);
    put(b, rnd(), 8);
    key(b, keys);
    key(b, keys);
    fill(b, 64);
  } else if (tag == 2) {
    header_body(b, keys);
    const uint64_t nv = below(12);
    put(b, nv, 8);
    for (uint64_t v = 0; v < nv; ++v) {
      key(b, keys);
      fill(b, 64);
    }
  } else {
    const uint64_t nd = below(5);
    put(b, nd, 8);
    fill(b, 32 * nd);
    key(b, keys);
  }
  return b;
}

}  // namespace

int main() {
  std::vector<std::string> keys;
  std::string texts;
  for (int k = 0; k < 6; ++k) {
    std::string s(43, 'A');
    for (char& c : s) c = (char)('A' + below(26));
    keys.push_back(s + "=");
    texts += keys.back();
  }
  std::vector<Bytes> seeds;
  for (int i = 0; i < 64; ++i) seeds.push_back(message((uint32_t)(i % 4), keys));
  const uint64_t big[] = {0, 1, 43, 44, 45, 1ull << 20, (1ull << 20) + 1, 1ull << 32, 1ull << 61, ~0ull};
  uint64_t decided[4] = {0, 0, 0, 0}, host = 0;
  for (int it = 0; it < 200000; ++it) {
    Bytes m = seeds[below(seeds.size())];
    switch (it % 6) {
      case 0: break;  // as built
      case 1:         // flip bits
        for (uint64_t k = 1 + below(5); k && !m.empty(); --k) m[below(m.size())] ^= (uint8_t)(1u << below(8));
        break;
      case 2: {       // overwrite a count / length region
        const uint64_t p = below(m.size() > 8 ? m.size() - 8 : 1), x = below(2) ? big[below(10)] : rnd();
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
      default:  // garbage behind a tag 0..4
        m.clear();
        put(m, below(5), 4);
        fill(m, below(300));
    }
    // a heap block of exactly the message's length: AddressSanitizer sees what the loader's check would miss
    uint8_t* blk = (uint8_t*)malloc(m.size() ? m.size() : 1);
    if (!m.empty()) memcpy(blk, m.data(), m.size());
    for (uint32_t kinds : {nt::kMsgKindsAll, nt::kMsgKindsCert}) {
      uint64_t f[15];
      ntmp_walk(blk, m.size(), kinds, (const uint8_t*)texts.data(), (uint32_t)keys.size(), f);
      if (f[0] == nt::kMsgHost) {
        host += kinds == nt::kMsgKindsAll;
        continue;
      }
      // a plan never reaches past the message, and only kinds asked for are decided
      if (f[14] > m.size() || !((kinds >> f[0]) & 1u) || f[0] != (uint32_t)(m[0] | m[1] << 8 | m[2] << 16 | m[3] << 24)) {
        fprintf(stderr, "msg_plan: iteration %d: a plan of kind %llu covers %llu bytes of %zu\n", it,
                (unsigned long long)f[0], (unsigned long long)f[14], m.size());
        abort();
      }
      if (kinds == nt::kMsgKindsAll && f[12]) decided[f[0]]++;
    }
    free(blk);
  }
  printf("msg_plan_check: decidable headers %llu votes %llu certificates %llu requests %llu, host %llu\n",
         (unsigned long long)decided[0], (unsigned long long)decided[1], (unsigned long long)decided[2],
         (unsigned long long)decided[3], (unsigned long long)host);
  // the unmutated sixth alone decides thousands of each kind
  for (int k = 0; k < 4; ++k)
    if (decided[k] < 1000) return 1;
  return 0;
}
#endif
