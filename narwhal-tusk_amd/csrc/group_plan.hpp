// group_plan.hpp -- the arithmetic of one shard of a certificate-groups call
// (host-only, no HIP: shared by groups.cpp and the host test harness).  A shard
// is groups [glo, ghi) of the caller's (first, cnt) arrays; its signatures are
// compacted chunk by chunk (pipe_plan.hpp plan_group_chunks), each chunk owning
// whole 64-bit words of the shard's signature verdicts.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "pipe_plan.hpp"

namespace nt {

struct GroupShard {
  uint64_t glo = 0, ghi = 0;
  std::vector<std::pair<uint64_t, uint64_t>> ch;  // chunk c = caller groups [ch[c].first, ch[c].second)
  std::vector<uint64_t> E, W;  // per chunk (C + 1 entries): first compacted signature, verdict-word base
  uint64_t* start = nullptr;  // per group g - glo: its first signature within its chunk (caller's storage,
                              // written chunk by chunk by fill_starts)
  uint64_t m = 0;          // signatures
  uint64_t sw = 0, gw = 0;  // signature / group verdict words
  uint64_t max_chunk = 0;  // signatures of the largest chunk
  bool direct = false;     // the groups lie back to back in the caller's arrays (and m > 0)

  size_t chunks() const { return ch.size(); }
  uint64_t groups() const { return ghi - glo; }
  uint64_t sigs(size_t c) const { return E[c + 1] - E[c]; }
  // THE map from (chunk, chunk-local signature) to a bit of the shard's signature verdict words
  uint64_t bit(size_t c, uint64_t e) const { return 64 * W[c] + e; }
  uint64_t bit(size_t c, uint64_t g, uint64_t t) const { return bit(c, start[g - glo] + t); }
  // Chunk c's group starts.  Left to the plan's user, chunk by chunk: the runtime
  // fills chunk c as it stages it, under the copies of the chunks before it
  // (100k groups up front cost a config-3 call 1.9 % in bench.py's host_api);
  // every chunk is filled before anything asks for bit(c, g, t).
  void fill_starts(size_t c, const uint32_t* cnt) const {
    uint64_t e = 0;
    for (uint64_t g = ch[c].first; g < ch[c].second; ++g) {
      start[g - glo] = e;
      e += cnt[g];
    }
  }
  void fill_starts(const uint32_t* cnt) const {
    for (size_t c = 0; c < chunks(); ++c) fill_starts(c, cnt);
  }
};

// The plan of groups [glo, ghi) cut into chunks of about targets[c] signatures.
// `start` takes the ghi - glo chunk-local group starts (fill_starts); the plan
// keeps the pointer (the runtime hands it pinned memory: the starts are copied
// to the device as they are).
inline GroupShard plan_group_shard(uint64_t glo, uint64_t ghi, const uint64_t* first, const uint32_t* cnt,
                                   const std::vector<uint64_t>& targets, uint64_t* start) {
  GroupShard p;
  p.glo = glo;
  p.ghi = ghi;
  p.ch = plan_group_chunks(glo, ghi, cnt, targets);
  p.start = start;
  const size_t C = p.ch.size();
  p.E.assign(C + 1, 0);
  p.W.assign(C + 1, 0);
  for (size_t c = 0; c < C; ++c) {
    uint64_t e = 0;
    for (uint64_t g = p.ch[c].first; g < p.ch[c].second; ++g) e += cnt[g];
    p.E[c + 1] = p.E[c] + e;
    p.W[c + 1] = p.W[c] + (e + 63) / 64;
    p.max_chunk = std::max(p.max_chunk, e);
  }
  p.m = p.E[C];
  p.sw = p.W[C];
  p.gw = (ghi - glo + 63) / 64;
  p.direct = p.m > 0;
  for (uint64_t g = glo; p.direct && g + 1 < ghi; ++g) p.direct = first[g + 1] == first[g] + cnt[g];
  return p;
}

// A signature whose key the registry index does not hold: caller group, the group's chunk, index within the group
struct GroupMiss {
  uint64_t g;
  uint32_t c;
  uint32_t t;
};

// The fallback kernel's verdicts mw (bit j = miss[j]) merged into the shard's
// verdict words: the misses' signature bits set in sbits, and the bits of
// exactly the groups that hold a miss recomputed in gbits (bit g - glo).
inline void merge_group_misses(const GroupShard& p, const uint32_t* cnt, const std::vector<GroupMiss>& miss,
                               const uint64_t* mw, uint64_t* sbits, uint64_t* gbits) {
  std::vector<std::pair<uint64_t, uint32_t>> groups;  // (group, chunk) of every miss
  for (size_t j = 0; j < miss.size(); ++j) {
    if (word_bit(mw, j)) word_put(sbits, p.bit(miss[j].c, miss[j].g, miss[j].t), true);
    groups.emplace_back(miss[j].g, miss[j].c);
  }
  std::sort(groups.begin(), groups.end());
  groups.erase(std::unique(groups.begin(), groups.end()), groups.end());
  for (const auto& gc : groups) {
    const uint64_t b0 = p.bit(gc.second, gc.first, 0);
    bool all = true;
    for (uint64_t t = 0; t < cnt[gc.first] && all; ++t) all = word_bit(sbits, b0 + t);
    word_put(gbits, gc.first - p.glo, all);
  }
}

// The shard's compacted signature bits ORed into the caller's bitmap: signature
// t of group g at bit first[g] + t (the caller zeroed the bitmap; bits of slots
// no group covers stay 0)
inline void scatter_sig_bits(const GroupShard& p, const uint64_t* first, const uint32_t* cnt, const uint64_t* sbits,
                             uint8_t* out) {
  for (size_t c = 0; c < p.chunks(); ++c)
    for (uint64_t g = p.ch[c].first; g < p.ch[c].second; ++g) {
      const uint64_t b0 = p.bit(c, g, 0);
      for (uint32_t t = 0; t < cnt[g]; ++t)
        if (word_bit(sbits, b0 + t)) byte_put(out, first[g] + t, true);
    }
}

}  // namespace nt
