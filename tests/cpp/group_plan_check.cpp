// group_plan_check.cpp -- TEST INFRASTRUCTURE: a stand-alone driver of
// narwhal-tusk_amd/csrc/group_plan.hpp for host sanitizer runs:
//   make -C tests/cpp build/group_plan_check && tests/cpp/build/group_plan_check
// (g++ -fsanitize=address,undefined -fno-sanitize-recover=all).
// It walks the shapes of tests/test_group_plan.py (G = 1 .. 1000, ragged and
// empty groups, shard starts off 0, dense and scattered layouts, 1 / 3 / 15
// chunk targets) through the plan, the miss merge and the scatter, every buffer
// allocated at exactly the size the runtime reserves, and compares with a
// recomputation from scratch.  Exit status 0 = clean.
#include <cstdio>
#include <cstdlib>

#include "../../narwhal-tusk_amd/csrc/group_plan.hpp"

using namespace nt;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static int check(uint64_t G, uint64_t glo, int nchunks, bool scattered) {
  std::vector<uint32_t> cnt(G);
  for (auto& c : cnt) c = (uint32_t)(rnd() % 30);
  if (G > 80) cnt[3] = cnt[77] = 0;
  std::vector<uint64_t> first(G);
  uint64_t pos = 0, nsig = 0;
  for (uint64_t i = 0; i < G; ++i) {
    const uint64_t g = scattered ? G - 1 - i : i;
    first[g] = pos;
    pos += cnt[g] + (scattered ? 3 : 0);
    nsig = std::max(nsig, first[g] + cnt[g]);
  }
  uint64_t total = 0;
  for (uint64_t g = glo; g < G; ++g) total += cnt[g];
  std::vector<uint64_t> targets(nchunks - 1, std::max<uint64_t>(64, total / nchunks / 64 * 64));
  targets.push_back(std::max<uint64_t>(total, 1));
  std::vector<uint64_t> start(G - glo);
  const GroupShard p = plan_group_shard(glo, G, first.data(), cnt.data(), targets, start.data());
  p.fill_starts(cnt.data());
  if (p.m != total || p.chunks() == 0 || p.ch.back().second != G) return 1;
  // verdicts: the truth, the misses (rejected by the first pass), the fallback's answers
  std::vector<uint64_t> sbits(p.sw, 0), gbits(p.gw, 0), want_s(p.sw, 0), want_g(p.gw, 0);
  std::vector<GroupMiss> miss;
  std::vector<uint8_t> fb;
  for (size_t c = 0; c < p.chunks(); ++c)
    for (uint64_t g = p.ch[c].first; g < p.ch[c].second; ++g) {
      bool all = true, want_all = true;
      for (uint32_t t = 0; t < cnt[g]; ++t) {
        const bool ok = rnd() % 10 != 0, m = rnd() % 5 == 0, f = rnd() % 3 != 0;
        if (p.bit(c, g, t) >= 64 * p.sw) return 2;
        if (m) {
          miss.push_back(GroupMiss{g, (uint32_t)c, t});
          fb.push_back(f);
        }
        if (ok && !m) word_put(sbits.data(), p.bit(c, g, t), true);
        if (m ? f : ok) word_put(want_s.data(), p.bit(c, g, t), true);
        all = all && ok && !m;
        want_all = want_all && (m ? f : ok);
      }
      word_put(gbits.data(), g - glo, all);
      word_put(want_g.data(), g - glo, want_all);
    }
  std::vector<uint64_t> mw((miss.size() + 63) / 64, 0);
  for (size_t j = 0; j < fb.size(); ++j) word_put(mw.data(), j, fb[j]);
  merge_group_misses(p, cnt.data(), miss, mw.data(), sbits.data(), gbits.data());
  if (sbits != want_s || gbits != want_g) return 3;
  std::vector<uint8_t> out((nsig + 7) / 8, 0), want_o((nsig + 7) / 8, 0);
  scatter_sig_bits(p, first.data(), cnt.data(), sbits.data(), out.data());
  for (size_t c = 0; c < p.chunks(); ++c)
    for (uint64_t g = p.ch[c].first; g < p.ch[c].second; ++g)
      for (uint32_t t = 0; t < cnt[g]; ++t)
        if (word_bit(want_s.data(), p.bit(c, g, t))) byte_put(want_o.data(), first[g] + t, true);
  return out == want_o ? 0 : 4;
}

int main() {
  int runs = 0;
  for (uint64_t G : {1, 63, 64, 65, 203, 1000})
    for (uint64_t glo : {(uint64_t)0, ((G - 1) / 64 + 1) / 2 * 64})
      for (int nchunks : {1, 3, 15})
        for (bool scattered : {false, true}) {
          const int rc = check(G, glo, nchunks, scattered);
          if (rc) {
            std::fprintf(stderr, "group_plan_check: G=%llu glo=%llu chunks=%d scattered=%d: failure %d\n",
                         (unsigned long long)G, (unsigned long long)glo, nchunks, (int)scattered, rc);
            return 1;
          }
          ++runs;
        }
  std::printf("group_plan_check: %d shapes ok\n", runs);
  return 0;
}
