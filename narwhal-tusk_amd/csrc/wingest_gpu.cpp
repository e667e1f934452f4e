// wingest_gpu.cpp -- C ABI of the worker's message ingestion from wire bytes
// (include/ntcrypto.h: nt_worker_messages_ingest; kernels in k_wingest.hip, the
// layout in wmsg_plan.hpp).  The call needs no key set and no committee, and
// builds no table: a worker verifies nothing.
//
// Per device shard the messages are cut into chunks BY BYTES (a worker's
// messages are 500 KB batches and 100-byte requests in one drain): equal byte
// shares of at most chunk_max_bytes, each closed at the first message boundary
// that reaches it, and at most the digest entry point's 65,536 messages.
// Chunk c's wire bytes and rebased offsets go over the copy stream into the
// buffers side[c % 3]; once the host has seen them land it launches, on compute
// lane c & 1: the walk (one wave per message), the SHA-512 launch over the same
// bytes with the lengths the walk wrote, the receipt kernel, and the copies of
// the codes and receipts back to pinned host memory.  From pinned input the
// copy of chunk c + 1 is queued before the host waits for chunk c's, so the
// link never idles; three sets of buffers, so that copy never waits for the
// two chunks whose kernels are in flight (a set is reused once the chunk three
// before has finished: its event).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/ntcrypto.h"
#include "pipeline.hpp"
#include "wingest.hpp"
#include "wmsg_plan.hpp"

using namespace ntrt;

static_assert(sizeof(nt_worker_receipt) == 4 * nt::kWmsgReceiptWords, "the record is wmsg_plan.hpp's 16 words");
static_assert(NT_WMSG_OK == nt::kWmsgOk && NT_WMSG_SERIALIZATION == nt::kWmsgSerialization &&
                  NT_WMSG_HOST == nt::kWmsgHost && NT_WORKER_RECEIPT_UNIFORM == nt::kWmsgUniform,
              "ntcrypto.h and wmsg_plan.hpp agree");

namespace {

using nt::kWmsgSlack;

struct Side {  // device buffers of one chunk in flight, grow-only
  DevBuf wire, moff, mlen, hlen, plan, sha, code, rec;
  hipEvent_t copied = nullptr;  // the chunk's inputs are on the device
  hipEvent_t done = nullptr;    // the chunk's kernels and copies back are finished
  ~Side() {
    for (hipEvent_t e : {copied, done})
      if (e) (void)hipEventDestroy(e);
  }
};

struct WingestState {  // goes with its slot (~Device has set the device)
  Side side[3];  // chunk c uses side[c % 3] on lane c & 1: a copy never waits for the two launches in flight
  HostBuf hoff, hlen, hcode, hrec;
};

struct Chunk {
  uint64_t a = 0, b = 0;        // messages [a, b) of the shard
  uint64_t base = 0, span = 0;  // host bytes [base, base + span)
  uint64_t lmax = 0;            // the longest message (selects the SHA-512 kernel)
};

// A positive integer from the environment, else dflt (unset, malformed or not positive).  The two
// variables below are test hooks (include/ntcrypto.h), read at every call so a test can set them.
uint64_t env_positive(const char* name, uint64_t dflt) {
  const char* e = std::getenv(name);
  if (!e) return dflt;
  char* end = nullptr;
  const long long v = std::strtoll(e, &end, 10);
  return end != e && *end == 0 && v > 0 ? (uint64_t)v : dflt;
}
// most messages of one chunk: the digest entry point's round (NT_WINGEST_CHUNK; tests force a few)
uint64_t chunk_max_msgs() { return env_positive("NT_WINGEST_CHUNK", 1 << 16); }
// Most bytes of one chunk.  A chunk's SHA-512 launch lasts as long as the serial chain of its
// longest message, whatever the chunk holds (one lane hashes ~30 MB/s: 17 ms for a 508 KB
// batch), and the two lanes run two launches at a time.  Chunks whose copy takes less than half
// a launch queue up behind each other: cut into 16 ramped chunks, 2 GB of batches took 262 ms
// against the digest call's 54 (profiles/ingest_worker/).  1024 x the longest message copies
// in ~0.6 launches at 52 GB/s; 64 MB at least, and 1 GB at most -- one multi-megabyte message
// in a drain must not turn the shard into one chunk and the grow-only buffers into the size of
// the drain (a longer message is a chunk of its own).  NT_WINGEST_CHUNK_BYTES sets it outright.
constexpr uint64_t kChunkBytesMin = 64ull << 20, kChunkBytesMax = 1ull << 30;
uint64_t chunk_max_bytes(uint64_t longest) {
  const uint64_t byl = longest > kChunkBytesMax / 1024 ? kChunkBytesMax : 1024 * longest;
  return env_positive("NT_WINGEST_CHUNK_BYTES", std::max(kChunkBytesMin, byl));
}

// messages [0, n) of a shard in chunks of equal byte shares, each closed at the first message
// boundary that reaches its share's end
std::vector<Chunk> plan_byte_chunks(const uint64_t* len, uint64_t n) {
  uint64_t total = 0, longest = 0;
  for (uint64_t i = 0; i < n; ++i) {
    total += len[i];
    longest = std::max(longest, len[i]);
  }
  const uint64_t cap = chunk_max_bytes(longest), K = std::max<uint64_t>(1, (total + cap - 1) / cap);
  const uint64_t share = std::max<uint64_t>(1, (total + K - 1) / K), mmax = chunk_max_msgs();
  std::vector<Chunk> ch;
  uint64_t acc = 0, goal = share;  // bytes so far; where the current share ends
  Chunk c;
  for (uint64_t i = 0; i < n; ++i) {
    acc += len[i];
    if (i + 1 - c.a >= mmax || acc >= goal) {
      c.b = i + 1;
      ch.push_back(c);
      c = Chunk{};
      c.a = i + 1;
      goal = (acc / share + 1) * share;
    }
  }
  if (c.a < n) {
    c.b = n;
    ch.push_back(c);
  }
  return ch;
}

// plain host loader of wmsg_plan.hpp (the small-call path)
struct HostLd {
  const uint8_t* p;
  uint32_t u8(uint64_t o) const { return p[o]; }
  uint32_t u32(uint64_t o) const {
    uint32_t x;
    std::memcpy(&x, p + o, 4);
    return x;
  }
  uint64_t u64(uint64_t o) const {
    uint64_t x;
    std::memcpy(&x, p + o, 8);
    return x;
  }
};

// one message on the host lane: the same walk, the host lane's SHA-512
void wingest_host_one(const uint8_t* msg, uint64_t L, uint8_t* code, nt_worker_receipt* rec) {
  uint8_t dig[32] = {0};
  const nt::WmsgPlan m = nt::wmsg_walk(HostLd{msg}, L, dig);
  *code = (uint8_t)m.code;
  if (!rec) return;
  if (m.code == nt::kWmsgOk && m.kind == nt::kWmsgBatch) nt::cpu::sha512_trunc32(msg, L, dig);
  uint32_t dw[8], w[nt::kWmsgReceiptWords];
  std::memcpy(dw, dig, 32);
  nt::wmsg_receipt_words(m, dw, w);
  std::memcpy(rec, w, sizeof w);
}

// the copies of chunk ch into sd, on the copy stream
int wingest_copy(Device& dv, WingestState& S, Side& sd, Chunk& ch, const uint8_t* data, const uint64_t* off,
                 const uint64_t* len, bool receipts) {
  const uint64_t m = ch.b - ch.a;
  uint64_t* ho = S.hoff.as<uint64_t>() + ch.a;
  uint64_t* hl = S.hlen.as<uint64_t>() + ch.a;
  uint64_t mn = UINT64_MAX, mx = 0;
  ch.lmax = 0;
  for (uint64_t i = ch.a; i < ch.b; ++i) {
    if (len[i] == 0) continue;
    mn = std::min(mn, off[i]);
    mx = std::max(mx, off[i] + len[i]);
    ch.lmax = std::max(ch.lmax, len[i]);
  }
  if (mn == UINT64_MAX) mn = mx = 0;
  ch.base = mn & ~(uint64_t)15;
  ch.span = mx - ch.base;
  for (uint64_t i = ch.a; i < ch.b; ++i) {
    ho[i - ch.a] = len[i] ? kWmsgSlack + off[i] - ch.base : kWmsgSlack;
    hl[i - ch.a] = len[i];
  }
  // the buffers' previous chunk has finished (the caller waited for sd.done): nothing uses these
  NT_CHK0(sd.wire.ensure(ch.span + 2 * kWmsgSlack));
  NT_CHK0(sd.moff.ensure(m * 8));
  NT_CHK0(sd.mlen.ensure(m * 8));
  NT_CHK0(sd.hlen.ensure(m * 8));
  NT_CHK0(sd.plan.ensure(m * sizeof(nt_worker_receipt)));
  NT_CHK0(sd.code.ensure(m));
  if (receipts) {
    NT_CHK0(sd.sha.ensure(m * 32));
    NT_CHK0(sd.rec.ensure(m * sizeof(nt_worker_receipt)));
  }
  if (ch.span)
    NT_TRY(hipMemcpyAsync(sd.wire.as<uint8_t>() + kWmsgSlack, data + ch.base, ch.span, hipMemcpyHostToDevice,
                          dv.cstream));
  NT_TRY(hipMemcpyAsync(sd.moff.p, ho, m * 8, hipMemcpyHostToDevice, dv.cstream));
  NT_TRY(hipMemcpyAsync(sd.mlen.p, hl, m * 8, hipMemcpyHostToDevice, dv.cstream));
  NT_TRY(hipEventRecord(sd.copied, dv.cstream));
  return NT_OK;
}

// the kernels of chunk ch on stream s, its codes and receipts back
int wingest_launch(WingestState& S, Side& sd, const Chunk& ch, bool receipts, hipStream_t s) {
  const uint64_t m = ch.b - ch.a;
  nt::WmsgBufs b{};
  b.wire = sd.wire.as<uint8_t>();
  b.wire_bytes = kWmsgSlack + ch.span;
  b.moff = sd.moff.as<uint64_t>();
  b.mlen = sd.mlen.as<uint64_t>();
  b.n = m;
  b.plan = sd.plan.as<uint4>();
  b.hlen = sd.hlen.as<uint64_t>();
  b.code = sd.code.as<uint8_t>();
  NT_TRY(nt::launch_wmsg_walk(b, s));
  NT_TRY(hipMemcpyAsync(S.hcode.as<uint8_t>() + ch.a, b.code, m, hipMemcpyDeviceToHost, s));
  if (receipts) {
    b.sha = sd.sha.as<uint8_t>();
    b.rec = sd.rec.as<uint4>();
    NT_TRY(nt::launch_sha512_trunc32(b.wire, b.wire_bytes, b.moff, b.hlen, m, sd.sha.as<uint8_t>(), s, ch.lmax));
    NT_TRY(nt::launch_wmsg_receipt(b, s));
    NT_TRY(hipMemcpyAsync(S.hrec.as<nt_worker_receipt>() + ch.a, b.rec, m * sizeof(nt_worker_receipt),
                          hipMemcpyDeviceToHost, s));
  }
  NT_TRY(hipEventRecord(sd.done, s));
  return NT_OK;
}

int wingest_shard(Device& dv, const uint8_t* data, const uint64_t* off, const uint64_t* len, uint64_t lo, uint64_t hi,
                  uint8_t* out_code, nt_worker_receipt* out_receipt) {
  const uint64_t n = hi - lo;
  if (!n) return NT_OK;
  if (!dv.wingest) {
    auto st = std::make_shared<WingestState>();
    for (auto& sd : st->side) {
      NT_TRY(hipEventCreateWithFlags(&sd.copied, hipEventDisableTiming));
      NT_TRY(hipEventCreateWithFlags(&sd.done, hipEventDisableTiming));
    }
    dv.wingest = st;
  }
  WingestState& S = *(WingestState*)dv.wingest.get();
  const bool receipts = out_receipt != nullptr;
  // both compute streams must be idle before the shared host staging is rewritten
  for (Lane& l : dv.lane) NT_TRY(hipStreamSynchronize(l.stream));
  NT_CHK0(S.hoff.ensure(n * 8));
  NT_CHK0(S.hlen.ensure(n * 8));
  NT_CHK0(S.hcode.ensure(n));
  if (receipts) NT_CHK0(S.hrec.ensure(n * sizeof(nt_worker_receipt)));
  const uint64_t* o = off + lo;
  const uint64_t* l = len + lo;
  std::vector<Chunk> ch = plan_byte_chunks(l, n);
  const size_t C = ch.size();
  bool async = true;  // every chunk's wire bytes lie in nt_host_alloc memory
  for (const Chunk& c : ch) {
    uint64_t mn = UINT64_MAX, mx = 0;
    for (uint64_t i = c.a; i < c.b; ++i) {
      if (l[i] == 0) continue;
      mn = std::min(mn, o[i]);
      mx = std::max(mx, o[i] + l[i]);
    }
    if (mn != UINT64_MAX && !is_pinned(data + mn, mx - mn)) async = false;
  }
  auto copy = [&](size_t c) -> int {
    Side& sd = S.side[c % 3];
    if (c >= 3) NT_TRY(hipEventSynchronize(sd.done));  // chunk c - 3 is finished with the buffers
    return wingest_copy(dv, S, sd, ch[c], data, o, l, receipts);
  };
  // pipeline.hpp run_chunks' order: the compute streams never hold a wait for the copy stream
  if (async) NT_CHK0(copy(0));
  for (size_t c = 0; c < C; ++c) {
    if (!async) NT_CHK0(copy(c));
    else if (c + 1 < C) NT_CHK0(copy(c + 1));
    Side& sd = S.side[c % 3];
    NT_TRY(hipEventSynchronize(sd.copied));
    NT_CHK0(wingest_launch(S, sd, ch[c], receipts, dv.cstr((int)c)));
  }
  for (Lane& ln : dv.lane) NT_TRY(hipStreamSynchronize(ln.stream));
  std::memcpy(out_code + lo, S.hcode.p, n);
  if (receipts) std::memcpy(out_receipt + lo, S.hrec.p, n * sizeof(nt_worker_receipt));
  return NT_OK;
}

}  // namespace

extern "C" {

int nt_worker_messages_ingest(nt_ctx* ctx, const uint8_t* data, const uint64_t* off, const uint64_t* len, uint64_t n,
                              uint8_t* out_code, nt_worker_receipt* out_receipt) {
  if (!ctx || (n && (!data || !off || !len || !out_code))) return NT_EINVAL;
  if (n == 0) return NT_OK;
  if (small_sha(ctx, n, len)) {
    nt::cpu::parallel_for(n, small_threads(ctx, n), [&](uint64_t i) {
      wingest_host_one(data + off[i], len[i], out_code + i, out_receipt ? out_receipt + i : nullptr);
    });
    ctx->calls_host++;
    return NT_OK;
  }
  ctx->calls_gpu++;
  return run_sharded(ctx, n, 1, [&](Device& dv, uint64_t lo, uint64_t hi) {
    return wingest_shard(dv, data, off, len, lo, hi, out_code, out_receipt);
  }, sha_latency(n, len));
}

}  // extern "C"
