// probe_entries_check.cpp -- TEST INFRASTRUCTURE: a stand-alone driver of the probe's shared
// per-item entry points (nt_probe_entries.inc) on the host runner, for host sanitizer runs:
//   make -C tests/cpp build/probe_entries_check && tests/cpp/build/probe_entries_check
// (g++ -fsanitize=address,undefined -fno-sanitize-recover=all).
// The harness is included whole, so the nthb_* entries here are the library's.  Every entry runs
// at n = 0, 1 and 65 on heap buffers of exactly n times the item's size, so that a wrong
// per-item size in an entry's description is an AddressSanitizer report, and its outputs (and
// key-table blob) are compared byte for byte with a direct loop over the same ntp::item_*.  Then
// every refusal of the argument checks: a non-zero return, outputs and blob left as they were.
// Exit status 0 = clean.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <initializer_list>
#include <vector>

#include "nt_host_harness.cpp"

static int fails = 0;
#define EXPECT(c)                                         \
  do {                                                    \
    if (!(c)) {                                           \
      std::printf("line %d: %s: %s\n", __LINE__, who, #c); \
      ++fails;                                            \
    }                                                     \
  } while (0)

namespace {
constexpr uint8_t kOutFill = 0xC3;
constexpr uint32_t kCap = 4;

// an exactly-sized heap allocation, handed out as whatever pointer the callee takes
struct Buf {
  uint8_t* p;
  size_t bytes;
  explicit Buf(size_t b, int fill = 0) : p((uint8_t*)std::malloc(b)), bytes(b) {
    if (b) std::memset(p, fill, b);
  }
  Buf(const Buf& o) : Buf(o.bytes) {
    if (bytes) std::memcpy(p, o.p, bytes);
  }
  Buf& operator=(const Buf&) = delete;
  ~Buf() { std::free(p); }
  template <class T>
  operator T*() const { return (T*)p; }
  uint32_t& w(size_t i) { return ((uint32_t*)p)[i]; }
  bool operator==(const Buf& o) const { return bytes == o.bytes && (bytes == 0 || std::memcmp(p, o.p, bytes) == 0); }
};

uint64_t g_x = 0x243f6a8885a308d3ull;
uint32_t rnd() {
  g_x ^= g_x << 13;
  g_x ^= g_x >> 7;
  g_x ^= g_x << 17;
  return (uint32_t)(g_x >> 16);
}
// n items of `words` random words, the last word of each ANDed with `top`
Buf words_of(uint64_t n, int words, uint32_t top = 0xffffffffu) {
  Buf b(4 * words * n);
  for (uint64_t i = 0; i < n; ++i)
    for (int l = 0; l < words; ++l) b.w(words * i + l) = rnd() & (l == words - 1 ? top : 0xffffffffu);
  return b;
}
Buf limbs_of(uint64_t n) {  // reduced limbs
  Buf b(40 * n);
  for (uint64_t i = 0; i < 10 * n; ++i) b.w(i) = rnd() & ((i % 10) & 1 ? NT_M25 : NT_M26);
  return b;
}
Buf small_of(uint64_t n, uint32_t bound) {  // n words below `bound`
  Buf b(4 * n);
  for (uint64_t i = 0; i < n; ++i) b.w(i) = rnd() % bound;
  return b;
}
// encodings that decode: y = 2, 3, ..., the first `distinct` of them in turn
Buf points_of(uint64_t n, uint32_t distinct) {
  static std::vector<uint32_t> ys;
  for (uint32_t y = 2; ys.size() < 16; ++y) {
    const uint32_t e[8] = {y};
    ge_p3 P;
    if (ge_frombytes_w(P, e)) ys.push_back(y);
  }
  Buf b(32 * n);
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t e[8] = {ys[i % distinct % 16]};
    std::memcpy(b.p + 32 * i, e, 32);
  }
  return b;
}
int bitlen(const uint32_t* w) {
  for (int b = 255; b >= 0; --b)
    if ((w[b >> 5] >> (b & 31)) & 1u) return b + 1;
  return 0;
}
// scalars of at most `bits` bits (a multiple of 32)
Buf short_of(uint64_t n, int bits) {
  Buf b(32 * n);
  for (uint64_t i = 0; i < n; ++i)
    for (int l = 0; l < bits / 32; ++l) b.w(8 * i + l) = rnd();
  return b;
}

using Outs = std::vector<Buf>;
using Call = std::function<int(Outs&, uint8_t*)>;
Outs outs_of(uint64_t n, std::initializer_list<size_t> per_item) {
  Outs o;
  for (size_t b : per_item) o.emplace_back(b * n, kOutFill);
  return o;
}
// the entry and the direct loop on their own outputs and their own copy of the blob
void both(const char* who, uint64_t n, std::initializer_list<size_t> per_item, const Buf& blob0, const Call& entry,
          const Call& direct) {
  Outs a = outs_of(n, per_item), b = outs_of(n, per_item);
  Buf ba(blob0), bb(blob0);
  EXPECT(entry(a, ba) == 0);
  direct(b, bb);
  EXPECT(a == b);
  EXPECT(ba == bb);
}
void refused(const char* who, uint64_t n, std::initializer_list<size_t> per_item, const Buf& blob0, const Call& entry) {
  Outs a = outs_of(n, per_item), b = outs_of(n, per_item);
  Buf ba(blob0);
  EXPECT(entry(a, ba) != 0);
  EXPECT(a == b);
  EXPECT(ba == blob0);
}
#define LOOP(call) \
  for (uint64_t i = 0; i < n; ++i) call; \
  return 0
#define LOOP_AT(call)                \
  for (uint64_t i = 0; i < n; ++i) { \
    HostATab at;                     \
    call;                            \
  }                                  \
  return 0

Buf empty_blob(bool comb) {
  Buf b(comb ? kcomb_probe_bytes(kCap) : ktab_probe_bytes(kCap), 0xA5);
  std::memset(b.p, 0, comb ? kKtProbePoolOff : b.bytes);
  return b;
}

void run_entries(uint64_t n, const Buf& ktab, const Buf& kcomb) {
  const Buf none(0);
  const Buf f = limbs_of(n), g = limbs_of(n), a = words_of(n, 8), b = words_of(n, 8), c = words_of(n, 8);
  const Buf k252 = words_of(n, 8, 0x0fffffffu), k253 = words_of(n, 8, 0x1fffffffu), x512 = words_of(n, 16);
  const Buf A = points_of(n, 4), R = points_of(n, 7), bit = small_of(n, 2), kidx = small_of(n, kCap);
  both("fe_mul", n, {40}, none, [&](Outs& o, uint8_t*) { return nthb_fe_mul(n, f, g, o[0]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_fe_mul(i, f, g, o[0])); });
  both("fe_sq", n, {40}, none, [&](Outs& o, uint8_t*) { return nthb_fe_sq(n, f, o[0]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_fe_sq(i, f, o[0])); });
  both("fe_sq_wide", n, {40}, none, [&](Outs& o, uint8_t*) { return nthb_fe_sq_wide(n, f, o[0]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_fe_sq_wide(i, f, o[0])); });
  both("fe_carry", n, {40}, none, [&](Outs& o, uint8_t*) { return nthb_fe_carry(n, f, o[0]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_fe_carry(i, f, o[0])); });
  both("fe_tobytes", n, {32}, none, [&](Outs& o, uint8_t*) { return nthb_fe_tobytes(n, f, o[0]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_fe_tobytes(i, f, o[0])); });
  both("fe_frombytes", n, {40}, none, [&](Outs& o, uint8_t*) { return nthb_fe_frombytes(n, a, o[0]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_fe_frombytes(i, a, o[0])); });
  both("sc_reduce512", n, {32}, none, [&](Outs& o, uint8_t*) { return nthb_sc_reduce512(n, x512, o[0]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_sc_reduce512(i, x512, o[0])); });
  both("sc_muladd", n, {32}, none, [&](Outs& o, uint8_t*) { return nthb_sc_muladd(n, a, b, c, o[0]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_sc_muladd(i, a, b, c, o[0])); });
  both("sc_mul", n, {32}, none, [&](Outs& o, uint8_t*) { return nthb_sc_mul(n, a, b, o[0]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_sc_mul(i, a, b, o[0])); });
  both("sc_reduce_half", n, {32, 4}, none, [&](Outs& o, uint8_t*) { return nthb_sc_reduce_half(n, k252, o[0], o[1]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_sc_reduce_half(i, k252, o[0], o[1])); });
  both("sc_recode_w4", n, {32}, none, [&](Outs& o, uint8_t*) { return nthb_sc_recode_w4(n, k252, o[0]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_sc_recode_w4(i, k252, o[0])); });
  both("sc_is_canonical", n, {4}, none, [&](Outs& o, uint8_t*) { return nthb_sc_is_canonical(n, a, o[0]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_sc_is_canonical(i, a, o[0])); });
  both("point_checks", n, {16}, none, [&](Outs& o, uint8_t*) { return nthb_point_checks(n, a, o[0]); },
       [&](Outs& o, uint8_t*) { LOOP(ntp::item_point_checks(i, a, o[0])); });
  for (int sw = 0; sw < 2; ++sw) {  // both values of each run-time switch
    both("fe_invert", n, {32}, none, [&](Outs& o, uint8_t*) { return nthb_fe_invert(n, f, o[0], sw); },
         [&](Outs& o, uint8_t*) { LOOP(ntp::item_fe_invert(i, f, o[0], sw)); });
    both("sc_halfsize", n, {32, 4, 32, 4}, none,
         [&](Outs& o, uint8_t*) { return nthb_sc_halfsize(n, k252, o[0], o[1], o[2], o[3], sw); },
         [&](Outs& o, uint8_t*) { LOOP(ntp::item_sc_halfsize(i, k252, o[0], o[1], o[2], o[3], sw)); });
    both("sc_unbalanced", n, {32, 4, 32, 4, 4}, none,
         [&](Outs& o, uint8_t*) { return nthb_sc_unbalanced(n, k252, o[0], o[1], o[2], o[3], o[4], sw); },
         [&](Outs& o, uint8_t*) { LOOP(ntp::item_sc_unbalanced(i, k252, o[0], o[1], o[2], o[3], o[4], sw)); });
  }
  {  // messages of 0 .. 64 bytes (32 among them: the one-block path) at every alignment, the last one ending the buffer
    Buf off(8 * n), len(8 * n);
    uint64_t end = 0;
    for (uint64_t i = 0; i < n; ++i) {
      ((uint64_t*)off)[i] = end + i % 8;
      ((uint64_t*)len)[i] = i % 3 == 0 ? 32 : i;
      end = ((uint64_t*)off)[i] + ((uint64_t*)len)[i];
    }
    const Buf msg = words_of((end + 3) / 4, 1);
    Buf exact(end);
    if (end) std::memcpy(exact.p, msg.p, end);
    for (int fast = 0; fast < 2; ++fast)
      both("hram", n, {32}, none, [&](Outs& o, uint8_t*) { return nthb_hram(n, a, b, exact, end, off, len, o[0], fast); },
           [&](Outs& o, uint8_t*) {
             std::vector<uint32_t> copy = form(Msg{exact, end});
             LOOP(ntp::item_hram(i, a, b, (const uint8_t*)copy.data(), off, len, o[0], fast));
           });
  }
  for (int bits : {kKeyCombNarrow, kKeyCombMid, kKeyCombWide, kKeyCombReduced, kBCombBits})
    both("wcomb_digits", n, {4 * kWcDigitWords}, none, [&](Outs& o, uint8_t*) { return nthb_wcomb_digits(bits, n, a, o[0]); },
         [&](Outs& o, uint8_t*) {
           wcomb_width(bits, [&](auto w) { for (uint64_t i = 0; i < n; ++i) ntp::item_wcomb_digits<decltype(w)::value>(i, a, o[0]); });
           return 0;
         });
  {  // the ladder: |u|, v of at most 128 bits, window counts of their own
    const Buf u = short_of(n, 128), v = short_of(n, 128);
    Buf bits(4 * n);
    for (uint64_t i = 0; i < n; ++i) ((int32_t*)bits)[i] = i % 5 == 4 ? 253 : 128 + (int)(i % 3);
    both("ladder_uv", n, {32}, none, [&](Outs& o, uint8_t*) { return nthb_ladder_uv(n, A, R, u, bit, v, bits, o[0]); },
         [&](Outs& o, uint8_t*) {
           LOOP_AT(ntp::item_ladder_uv(i, A, R, u, bit, v, bits, at, o[0], true));
         });
  }
  // the three-table items: fills of an empty table, then reads and ladders over the filled one
  both("ktab_fill", n, {4}, empty_blob(false), [&](Outs& o, uint8_t* bl) { return nthb_ktab_fill(n, A, bl, kCap, o[0]); },
       [&](Outs& o, uint8_t* bl) {
         const HostKTab kt = form(Blob<false>{bl, kCap});
         LOOP(ntp::item_ktab_fill(i, A, kt, o[0], true));
       });
  {
    Buf td(8 * n), sc4(16 * n);
    const Buf u = short_of(n, 192), v = short_of(n, 64);
    for (uint64_t i = 0; i < n; ++i) {
      ((int32_t*)td)[2 * i] = (int32_t)(i % kKtTables);
      ((int32_t*)td)[2 * i + 1] = (int32_t)(i % 17) - 8;
      const uint32_t s[4] = {rnd() & 1u, (uint32_t)bitlen((uint32_t*)u + 8 * i), (uint32_t)bitlen((uint32_t*)v + 8 * i), i % 7 == 6};
      std::memcpy(sc4.p + 16 * i, s, 16);
    }
    both("ktab_point", n, {12, 32}, ktab, [&](Outs& o, uint8_t* bl) { return nthb_ktab_point(n, A, td, bl, kCap, o[0], o[1]); },
         [&](Outs& o, uint8_t* bl) {
           const HostKTab kt = form(Blob<false>{bl, kCap});
           LOOP(ntp::item_ktab_point(i, A, td, kt, o[0], o[1]));
         });
    both("ladder_uv3", n, {32}, ktab, [&](Outs& o, uint8_t* bl) { return nthb_ladder_uv3(n, kidx, R, u, v, sc4, bl, kCap, o[0]); },
         [&](Outs& o, uint8_t* bl) {
           const HostKTab kt = form(Blob<false>{bl, kCap});
           LOOP_AT(ntp::item_ladder_uv3(i, kidx, R, u, v, sc4, at, kt, o[0], true));
         });
  }
  // the comb items, the same way
  both("kcomb_fill", n, {4}, empty_blob(true), [&](Outs& o, uint8_t* bl) { return nthb_kcomb_fill(n, A, bl, kCap, o[0]); },
       [&](Outs& o, uint8_t* bl) {
         const HostKComb kt = form(Blob<true>{bl, kCap});
         LOOP_AT(ntp::item_kcomb_fill(i, A, kt, at, o[0], true));
       });
  {
    const Buf line = small_of(n, 40), z = words_of(n, 8, 0x7fffffffu), flags = small_of(n, 4);
    for (uint64_t i = 0; i < n; ++i) z.p[32 * i] |= 1;  // z != 0
    both("kcomb_line", n, {12, 120}, kcomb, [&](Outs& o, uint8_t* bl) { return nthb_kcomb_line(n, A, line, bl, kCap, o[0], o[1]); },
         [&](Outs& o, uint8_t* bl) {
           const HostKComb kt = form(Blob<true>{bl, kCap});
           LOOP(ntp::item_kcomb_line(i, A, line, kt, o[0], o[1]));
         });
    both("kc_picks", n, {4 * kKcPickWords}, none, [&](Outs& o, uint8_t*) { return nthb_kc_picks(n, k253, o[0]); },
         [&](Outs& o, uint8_t*) {
           const HostKComb kt = form(NoTable{});
           LOOP(ntp::item_kc_picks(i, k253, kt, o[0]));
         });
    both("ladder_kc", n, {32}, kcomb, [&](Outs& o, uint8_t* bl) { return nthb_ladder_kc(n, kidx, k253, bit, bl, kCap, o[0]); },
         [&](Outs& o, uint8_t* bl) {
           const HostKComb kt = form(Blob<true>{bl, kCap});
           LOOP(ntp::item_ladder_kc(i, kidx, k253, bit, kt, o[0], true));
         });
    both("compare_one", n, {4}, none, [&](Outs& o, uint8_t*) { return nthb_compare_one(n, a, b, z, R, bit, o[0]); },
         [&](Outs& o, uint8_t*) { LOOP(ntp::item_compare_one(i, a, b, z, R, bit, o[0])); });
    both("verify_kc", n, {4}, kcomb,
         [&](Outs& o, uint8_t* bl) { return nthb_verify_kc(n, kidx, flags, R, k252, k253, bit, bl, kCap, o[0]); },
         [&](Outs& o, uint8_t* bl) {
           const HostKComb kt = form(Blob<true>{bl, kCap});
           const auto wb = live_bcomb();
           LOOP(ntp::item_verify_kc(i, kidx, flags, R, k252, k253, bit, wb, kt, o[0], true));
         });
  }
}

// every refusal, the offending item last of n = 65 valid ones
void run_refusals(const Buf& ktab, const Buf& kcomb) {
  const uint64_t n = 65, last = n - 1;
  const Buf none(0), A = points_of(n, 4), R = points_of(n, 7), a = words_of(n, 8), b = words_of(n, 8);
  const Buf k252 = words_of(n, 8, 0x0fffffffu), k253 = words_of(n, 8, 0x1fffffffu), u = short_of(n, 128), v = short_of(n, 64);
  const Buf z = words_of(n, 8, 0x7fffffffu);
  const uint32_t bad_caps[2] = {0, kKtProbeMaxCap + 1};
  auto with = [&](const Buf& base, size_t word, uint32_t value) {  // a copy with one word replaced
    Buf c(base);
    c.w(word) = value;
    return c;
  };
  {
    const Buf bits = small_of(n, 254), uneg = small_of(n, 2);
    for (uint32_t bad : {(uint32_t)-1, 254u}) {
      const Buf bb = with(bits, last, bad);
      refused("ladder_uv bits", n, {32}, none, [&](Outs& o, uint8_t*) { return nthb_ladder_uv(n, A, R, u, uneg, v, bb, o[0]); });
    }
  }
  {
    Buf off(8 * n), len(8 * n);  // 65 messages of 4 bytes in a buffer of 260
    for (uint64_t i = 0; i < n; ++i) { ((uint64_t*)off)[i] = 4 * i; ((uint64_t*)len)[i] = 4; }
    const Buf msg = words_of(n, 1);
    const uint64_t bad[3][2] = {{4 * last, 5}, {261, 0}, {~0ull - 1, 4}};  // past the end, start past the end, off + len wraps
    for (auto& ol : bad) {
      Buf o2(off), l2(len);
      ((uint64_t*)o2)[last] = ol[0];
      ((uint64_t*)l2)[last] = ol[1];
      for (int fast = 0; fast < 2; ++fast)
        refused("hram slice", n, {32}, none, [&](Outs& o, uint8_t*) { return nthb_hram(n, a, b, msg, 4 * n, o2, l2, o[0], fast); });
    }
  }
  refused("wcomb_digits width", n, {4 * kWcDigitWords}, none, [&](Outs& o, uint8_t*) { return nthb_wcomb_digits(17, n, a, o[0]); });
  const Buf kidx = small_of(n, kCap), bit = small_of(n, 2), flags = small_of(n, 4), line = small_of(n, 40);
  Buf td(8 * n), sc4(16 * n);
  for (uint64_t i = 0; i < n; ++i) {
    ((int32_t*)td)[2 * i] = (int32_t)(i % kKtTables);
    ((int32_t*)td)[2 * i + 1] = (int32_t)(i % 17) - 8;
    const uint32_t s[4] = {0, 128, 64, 0};
    std::memcpy(sc4.p + 16 * i, s, 16);
  }
  for (uint32_t cap : bad_caps) {
    refused("ktab_fill capacity", n, {4}, ktab, [&](Outs& o, uint8_t* bl) { return nthb_ktab_fill(n, A, bl, cap, o[0]); });
    refused("ktab_point capacity", n, {12, 32}, ktab, [&](Outs& o, uint8_t* bl) { return nthb_ktab_point(n, A, td, bl, cap, o[0], o[1]); });
    refused("ladder_uv3 capacity", n, {32}, ktab, [&](Outs& o, uint8_t* bl) { return nthb_ladder_uv3(n, kidx, R, u, v, sc4, bl, cap, o[0]); });
    refused("kcomb_fill capacity", n, {4}, kcomb, [&](Outs& o, uint8_t* bl) { return nthb_kcomb_fill(n, A, bl, cap, o[0]); });
    refused("kcomb_line capacity", n, {12, 120}, kcomb, [&](Outs& o, uint8_t* bl) { return nthb_kcomb_line(n, A, line, bl, cap, o[0], o[1]); });
    refused("ladder_kc capacity", n, {32}, kcomb, [&](Outs& o, uint8_t* bl) { return nthb_ladder_kc(n, kidx, k253, bit, bl, cap, o[0]); });
    refused("verify_kc capacity", n, {4}, kcomb,
            [&](Outs& o, uint8_t* bl) { return nthb_verify_kc(n, kidx, flags, R, k252, k253, bit, bl, cap, o[0]); });
  }
  const uint32_t bad_td[4][2] = {{(uint32_t)-1, 0}, {kKtTables, 0}, {0, (uint32_t)-9}, {0, 9}};
  for (auto& t : bad_td) {
    const Buf t2 = with(with(td, 2 * last, t[0]), 2 * last + 1, t[1]);
    refused("ktab_point table or digit", n, {12, 32}, ktab, [&](Outs& o, uint8_t* bl) { return nthb_ktab_point(n, A, t2, bl, kCap, o[0], o[1]); });
  }
  refused("ladder_uv3 entry", n, {32}, ktab,
          [&](Outs& o, uint8_t* bl) { return nthb_ladder_uv3(n, with(kidx, last, kCap), R, u, v, sc4, bl, kCap, o[0]); });
  const uint32_t bad_sc[4] = {2, 254, 254, 2};
  for (int j = 0; j < 4; ++j)
    refused("ladder_uv3 flags or lengths", n, {32}, ktab, [&](Outs& o, uint8_t* bl) {
      return nthb_ladder_uv3(n, kidx, R, u, v, with(sc4, 4 * last + j, bad_sc[j]), bl, kCap, o[0]);
    });
  const Buf k_big = with(k253, 8 * last + 7, 0x20000000u);  // 2^253
  refused("kc_picks scalar", n, {4 * kKcPickWords}, none, [&](Outs& o, uint8_t*) { return nthb_kc_picks(n, k_big, o[0]); });
  refused("ladder_kc scalar", n, {32}, kcomb, [&](Outs& o, uint8_t* bl) { return nthb_ladder_kc(n, kidx, k_big, bit, bl, kCap, o[0]); });
  refused("ladder_kc entry", n, {32}, kcomb,
          [&](Outs& o, uint8_t* bl) { return nthb_ladder_kc(n, with(kidx, last, kCap), k253, bit, bl, kCap, o[0]); });
  refused("ladder_kc dead", n, {32}, kcomb,
          [&](Outs& o, uint8_t* bl) { return nthb_ladder_kc(n, kidx, k253, with(bit, last, 2), bl, kCap, o[0]); });
  refused("compare_one mode", n, {4}, none,
          [&](Outs& o, uint8_t*) { return nthb_compare_one(n, a, b, z, R, with(bit, last, 2), o[0]); });
  auto vkc = [&](const Buf& ki, const Buf& kf, const Buf& S, const Buf& k, const Buf& mode) {
    return [&](Outs& o, uint8_t* bl) { return nthb_verify_kc(n, ki, kf, R, S, k, mode, bl, kCap, o[0]); };
  };
  {
    const Buf ki = with(kidx, last, kCap), kf = with(flags, last, 4), mode = with(bit, last, 2);
    refused("verify_kc entry", n, {4}, kcomb, vkc(ki, flags, k252, k253, bit));
    refused("verify_kc flags", n, {4}, kcomb, vkc(kidx, kf, k252, k253, bit));
    refused("verify_kc k", n, {4}, kcomb, vkc(kidx, flags, k252, k_big, bit));
    refused("verify_kc mode", n, {4}, kcomb, vkc(kidx, flags, k252, k253, mode));
    // (no s is refused: the 17 positions of the 16-bit comb hold any 256-bit scalar)
  }
  // the comb of B: a live set of another width, then none
  uint32_t meta[1];
  const char* who = "verify_kc comb of B";
  EXPECT(nthb_wcomb_build(kKeyCombMid, 1, kBaseEnc, 0, 1, meta) == 0);
  refused(who, n, {4}, kcomb, vkc(kidx, flags, k252, k253, bit));
  EXPECT(nthb_wcomb_free() == 0);
  refused(who, n, {4}, kcomb, vkc(kidx, flags, k252, k253, bit));
}
}  // namespace

int main() {
  const char* who = "setup";
  // the filled tables the readers and ladders run over: 4 keys, 4 entries, and the comb of B
  const Buf A = points_of(65, 4);
  Buf ktab = empty_blob(false), kcomb = empty_blob(true), slot(4 * 65);
  EXPECT(nthb_ktab_fill(65, A, ktab, kCap, slot) == 0 && ((uint32_t*)ktab)[0] == kCap);
  EXPECT(nthb_kcomb_fill(65, A, kcomb, kCap, slot) == 0 && ((uint32_t*)kcomb)[0] == kCap);
  uint32_t meta[1];
  EXPECT(nthb_wcomb_build(kKeyCombNarrow, 1, kBaseEnc, 0, 1, meta) == 0);
  for (uint64_t n : {0, 1, 65}) run_entries(n, ktab, kcomb);
  run_refusals(ktab, kcomb);
  if (fails) {
    std::printf("probe_entries_check: %d failures\n", fails);
    return 1;
  }
  std::printf("probe_entries_check: 28 entries at n = 0, 1, 65 and their refusals: clean\n");
  return 0;
}
