// wmsg_plan.hpp -- the layout walk of one bincode WorkerMessage (bincode 1.x,
// fixint, little endian; worker/src/worker.rs:270-292): the pure integer part
// of the worker's ingestion (k_wingest.hip k_wmsg_walk on the device, the host
// lane of wingest_gpu.cpp, host/narwhal.cpp worker::decode_message's check),
// compiled for the device and for the host (tests/cpp/wmsgplan/ runs it under
// the sanitizers over mutated messages).  Bytes are read through a loader
// functor -- ld.u8(off), ld.u32(off), ld.u64(off) -- and every count and offset
// is bounded by the message length before it is used: the walk reads nothing
// outside [0, len), and no offset wraps.
//
//   Batch         u32 0 | u64 ntx | ntx x (u64 len_k | len_k bytes)
//   BatchRequest  u32 1 | u64 nd  | nd x digest 32 | u64 44 | requestor b64 (44)
// Bytes after a complete message are allowed.
//
// Codes, in the order the checks are made:
//   kWmsgSerialization  bincode fails on the structure: len < 4, a tag above 1,
//                       no room for the count, a count that cannot fit (ntx
//                       prefixes of 8 bytes / nd digests of 32 do not fit in
//                       what is left), a length prefix or a string that runs
//                       past the end.  Compared before anything is added.
//   kWmsgHost           the device does not decide: a count that fits but is
//                       above the caps; a requestor string whose length prefix
//                       is not 44 (and does not run past the end), or whose 44
//                       characters are not the canonical base64 text of 32
//                       bytes (43 alphabet characters and '=', trailing bits
//                       zero) -- older base64 decoders accept other texts, and
//                       the host decoder keeps that question.
//   kWmsgOk             everything else.
//
// A batch is a pointer chase; it is walked by proven speculation, W = 64
// transactions per round (wmsg_round_*).  With hypothesis h for the length of
// the next transactions, lane j reads the prefix at p + j (8 + h) when that
// whole prefix lies inside the message.  Lane 0 reads at p itself, so its
// prefix s is the true one whatever h was, and it is checked as the serial
// rule would (room for the prefix, s <= len - p - 8).  If s == h, lane j
// agrees when its prefix is s and its transaction ends inside the message; the
// leading run of agreeing lanes is proven, since each one's position follows
// from the ones before it.  A lane that agrees behind a disagreeing one -- a
// coincidence inside transaction data -- proves nothing and is not counted.  If
// s != h only lane 0 is proven, and the next hypothesis is s.  Otherwise it is
// the prefix of the first lane that disagreed (it sits on a proven boundary),
// or s again when every lane agreed or that lane read nothing.  Each round
// proves at least one transaction: the walk is exact and ends in at most ntx
// rounds; a uniform batch takes ntx / 64 rounds of one load each.
#pragma once
#include <stdint.h>

#include "nt_common.hpp"

namespace nt {

constexpr uint32_t kWmsgOk = 0, kWmsgSerialization = 9, kWmsgHost = 0xffu;
constexpr uint32_t kWmsgBatch = 0, kWmsgRequest = 1, kWmsgNone = 0xffu;  // WmsgPlan::kind
constexpr uint32_t kWmsgUniform = 1u;                                     // flags bit 0
constexpr uint64_t kWmsgMaxDigests = 1u << 20;                            // larger requests go to the host decoder
constexpr uint64_t kWmsgMaxTx = 1u << 24;                                 // larger batches (ditto)
constexpr uint64_t kWmsgKeyChars = 44;                                    // base64 (padded) of 32 bytes
constexpr uint64_t kWmsgMaxLen = 1ull << 56;  // longer "messages" are not walked (63 strides must not wrap)
constexpr uint32_t kWmsgLanes = 64;
constexpr uint32_t kWmsgReceiptWords = 16;

// What the walk knows about one message (the receipt's fields, ntcrypto.h nt_worker_receipt).
struct WmsgPlan {
  uint32_t code = kWmsgSerialization, kind = kWmsgNone, flags = 0;
  uint32_t n = 0;       // transactions / digests
  uint64_t used = 0;    // bytes the decoder consumes
  uint64_t tx_bytes = 0;
  uint32_t tx_len = 0, off_key = 0;
};

NT_HD NT_INLINE WmsgPlan wmsg_fail(uint32_t code) {
  WmsgPlan m;
  m.code = code;
  return m;
}

// ---- the batch walk ----
struct WmsgWalk {
  uint64_t p = 12;       // the next transaction's prefix
  uint64_t r = 0;        // transactions left
  uint64_t h = 0;        // hypothesis: their length
  uint64_t tx_bytes = 0;
  uint64_t common = 0;   // length of the first transaction
  uint32_t uniform = 1;  // every transaction so far has length `common`
  uint32_t first = 1;    // none proven yet
  uint32_t err = 0;      // the serial rule failed: kWmsgSerialization
};

// Where lane j < min(64, r) reads its prefix in this round; false when that prefix does not
// lie wholly inside the message (the lane then loads nothing).  L < kWmsgMaxLen.
NT_HD NT_INLINE bool wmsg_lane_at(const WmsgWalk& w, uint64_t L, uint32_t j, uint64_t* q) {
  *q = w.p;
  if (j >= w.r || L - w.p < 8) return false;  // p <= L always
  if (j == 0) return true;
  const uint64_t room = L - w.p - 8;           // the last position a prefix may start at, from p
  if (w.h > room) return false;                // one stride already leaves the message (h may be any u64)
  const uint64_t d = (uint64_t)j * (8 + w.h);  // < 64 * 2^56 + 512: no wrap
  if (d > room) return false;
  *q = w.p + d;
  return true;
}

// Lane j's vote: it read v at q (valid), lane 0 read s.  Lane 0 always agrees with itself
// when the serial rule holds for it.
NT_HD NT_INLINE bool wmsg_lane_agrees(const WmsgWalk& w, uint64_t L, uint32_t j, bool valid, uint64_t q, uint64_t v,
                                      uint64_t s) {
  if (!valid || v != s || s > L - q - 8) return false;  // q + 8 <= L (valid)
  return j == 0 || s == w.h;
}

// Close the round.  valid0 / s: lane 0's; agree: bit j = lane j's vote; k_valid / k_v: the
// first disagreeing lane's (k = the number of trailing ones of agree, < 64) -- ignored
// when every lane agreed.
NT_HD NT_INLINE void wmsg_round_end(WmsgWalk& w, bool valid0, uint64_t s, uint64_t agree, bool k_valid,
                                    uint64_t k_v) {
  if (!valid0 || !(agree & 1u)) {  // no room for the prefix, or the transaction runs past the end
    w.err = 1;
    w.r = 0;
    return;
  }
  const uint64_t na = ~agree;
  uint64_t run = na ? (uint64_t)__builtin_ctzll(na) : 64u;
  if (run > w.r) run = w.r;  // lanes >= r never vote, so this only guards
  if (w.first) {
    w.common = s;
    w.first = 0;
  } else if (s != w.common) {
    w.uniform = 0;
  }
  // the lanes behind lane 0 sat on boundaries only if the hypothesis was right
  const bool on_boundary = s == w.h && run < 64 && k_valid;
  w.p += run * (8 + s);  // every proven transaction ends inside the message
  w.r -= run;
  w.tx_bytes += run * s;
  w.h = on_boundary ? k_v : s;
}

// ---- the requestor's key text ----
// 6-bit value of a standard-alphabet character, 0xff if it is none
NT_HD NT_INLINE uint32_t wmsg_b64_val(uint32_t c) {
  if (c - 'A' < 26u) return c - 'A';
  if (c - 'a' < 26u) return c - 'a' + 26;
  if (c - '0' < 10u) return c - '0' + 52;
  return c == '+' ? 62u : c == '/' ? 63u : 0xffu;
}
// character t < 44 of a canonical text: 43 alphabet characters (the last with its two
// trailing bits zero) and '='
NT_HD NT_INLINE bool wmsg_b64_char_ok(uint32_t t, uint32_t c) {
  if (t == 43) return c == '=';
  const uint32_t v = wmsg_b64_val(c);
  return v != 0xffu && (t != 42 || (v & 3u) == 0);
}
// byte b < 32 of the key from the 6-bit values of characters 4 (b / 3) + b % 3 and the next
NT_HD NT_INLINE uint32_t wmsg_b64_byte(uint32_t b, uint32_t v0, uint32_t v1) {
  const uint32_t r = b % 3;
  return r == 0 ? ((v0 << 2) | (v1 >> 4)) & 0xffu : r == 1 ? ((v0 << 4) | (v1 >> 2)) & 0xffu : ((v0 << 6) | v1) & 0xffu;
}
NT_HD NT_INLINE uint32_t wmsg_b64_first_char(uint32_t b) { return 4 * (b / 3) + b % 3; }

// ---- everything but the batch's pointer chase and the key text ----
// The message's head: the code if it is decided here (m.code != kWmsgOk, or a request's
// layout complete); for a batch m.kind = kWmsgBatch with m.n set and the walk left to do
// (wmsg_round_*), which wmsg_batch_done turns into the plan.
template <class Ld>
NT_HD NT_INLINE WmsgPlan wmsg_head(const Ld& ld, uint64_t L) {
  if (L < 4) return wmsg_fail(kWmsgSerialization);
  const uint32_t tag = ld.u32(0);
  if (tag > 1 || L < 12) return wmsg_fail(kWmsgSerialization);
  if (L >= kWmsgMaxLen) return wmsg_fail(kWmsgHost);
  const uint64_t cnt = ld.u64(4);
  WmsgPlan m;
  if (tag == kWmsgBatch) {
    if (cnt > (L - 12) / 8) return wmsg_fail(kWmsgSerialization);  // every transaction has a prefix
    if (cnt > kWmsgMaxTx) return wmsg_fail(kWmsgHost);
    m.code = kWmsgOk;
    m.kind = kWmsgBatch;
    m.n = (uint32_t)cnt;
    return m;
  }
  if (cnt > (L - 12) / 32) return wmsg_fail(kWmsgSerialization);
  if (cnt > kWmsgMaxDigests) return wmsg_fail(kWmsgHost);
  const uint64_t pos = 12 + 32 * cnt;
  if (L - pos < 8) return wmsg_fail(kWmsgSerialization);
  const uint64_t klen = ld.u64(pos);
  if (klen > L - pos - 8) return wmsg_fail(kWmsgSerialization);  // the string runs past the end
  if (klen != kWmsgKeyChars) return wmsg_fail(kWmsgHost);
  m.code = kWmsgOk;
  m.kind = kWmsgRequest;
  m.n = (uint32_t)cnt;
  m.used = pos + 8 + kWmsgKeyChars;
  m.off_key = (uint32_t)(pos + 8);  // < 12 + 2^25 + 8
  return m;
}

NT_HD NT_INLINE WmsgWalk wmsg_walk_start(const WmsgPlan& head) {
  WmsgWalk w;
  w.r = head.n;
  return w;
}

NT_HD NT_INLINE WmsgPlan wmsg_batch_done(const WmsgPlan& head, const WmsgWalk& w) {
  if (w.err) return wmsg_fail(kWmsgSerialization);
  WmsgPlan m = head;
  m.used = w.p;
  m.tx_bytes = w.tx_bytes;
  // the common length is reported in 32 bits; a (4 GB) longer one is not flagged
  if (head.n >= 1 && w.uniform && w.common <= 0xffffffffull) {
    m.flags = kWmsgUniform;
    m.tx_len = (uint32_t)w.common;
  }
  return m;
}

// The record (ntcrypto.h nt_worker_receipt) as 16 little-endian words = four 16-byte rows:
//   0  code | kind << 8 | flags << 16    4, 5  tx_bytes    8..15  digest
//   1  n                                 6     tx_len
//   2, 3  used                           7     off_key
// dig: the 8 digest words of an OK message (a batch's SHA-512[..32], a request's raw key);
// not read otherwise.
NT_HD NT_INLINE void wmsg_receipt_words(const WmsgPlan& m, const uint32_t dig[8], uint32_t w[kWmsgReceiptWords]) {
#pragma unroll
  for (uint32_t k = 0; k < kWmsgReceiptWords; ++k) w[k] = 0;
  if (m.code != kWmsgOk) {
    w[0] = (m.code & 0xffu) | (kWmsgNone << 8);
    return;
  }
  w[0] = kWmsgOk | (m.kind << 8) | (m.flags << 16);
  w[1] = m.n;
  w[2] = (uint32_t)m.used;
  w[3] = (uint32_t)(m.used >> 32);
  w[4] = (uint32_t)m.tx_bytes;
  w[5] = (uint32_t)(m.tx_bytes >> 32);
  w[6] = m.tx_len;
  w[7] = m.off_key;
#pragma unroll
  for (int j = 0; j < 8; ++j) w[8 + j] = dig[j];
}

// ---- the whole walk on one thread, W = 64 lanes in a loop (the host lane, the host
// decoder's check and the sanitized checker run the rounds the device runs) ----
// key32: the requestor's raw key of an OK request (untouched otherwise).  *rounds
// (nullable): the batch walk's rounds.
template <class Ld>
NT_HD NT_INLINE WmsgPlan wmsg_walk(const Ld& ld, uint64_t L, uint8_t key32[32], uint64_t* rounds = nullptr) {
  WmsgPlan m = wmsg_head(ld, L);
  if (rounds) *rounds = 0;
  if (m.code != kWmsgOk) return m;
  if (m.kind == kWmsgRequest) {
    uint32_t v[kWmsgKeyChars];
    bool ok = true;
    for (uint32_t t = 0; t < kWmsgKeyChars; ++t) {
      const uint32_t c = ld.u8(m.off_key + t);
      ok = ok && wmsg_b64_char_ok(t, c);
      v[t] = wmsg_b64_val(c);
    }
    if (!ok) return wmsg_fail(kWmsgHost);
    for (uint32_t b = 0; b < 32; ++b) {
      const uint32_t t = wmsg_b64_first_char(b);
      key32[b] = (uint8_t)wmsg_b64_byte(b, v[t], v[t + 1]);
    }
    return m;
  }
  WmsgWalk w = wmsg_walk_start(m);
  while (w.r) {
    uint64_t q[kWmsgLanes], v[kWmsgLanes], agree = 0;
    bool valid[kWmsgLanes];
    for (uint32_t j = 0; j < kWmsgLanes; ++j) {
      valid[j] = wmsg_lane_at(w, L, j, &q[j]);
      v[j] = valid[j] ? ld.u64(q[j]) : 0;
    }
    for (uint32_t j = 0; j < kWmsgLanes; ++j)
      if (wmsg_lane_agrees(w, L, j, valid[j], q[j], v[j], v[0])) agree |= 1ull << j;
    const uint64_t na = ~agree;
    const uint32_t k = na ? (uint32_t)__builtin_ctzll(na) : 0u;
    wmsg_round_end(w, valid[0], v[0], agree, valid[k], v[k]);
    if (rounds) ++*rounds;
  }
  return wmsg_batch_done(m, w);
}

}  // namespace nt
