// pipeline.hpp -- the chunk pipeline of the host entry points (verify.cpp,
// groups.cpp, sign.cpp): message staging, the copy / launch orders and the
// NT_PIPE_* switches.  Not part of the ABI.
//
// A shard's items are split into up to kMaxChunks contiguous chunks (multiples
// of 64 items, so each chunk owns whole 64-bit verdict words).  Chunk c's inputs
// are copied on the copy stream, and its kernels wait only for those copies:
// the PCIe transfer of chunk c+1 runs under the kernels of chunk c instead of
// before all of them.  NT_PIPE_CHUNKS caps the count (1 = one copy, one launch;
// default kMaxChunks).
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstdio>

#include "cpu_lane.hpp"
#include "pipe_plan.hpp"
#include "runtime.hpp"

namespace ntrt {

using nt::kMaxChunks;
using Chunks = std::vector<std::pair<uint64_t, uint64_t>>;

inline void words_to_bitmap(uint8_t* out, const uint64_t* words, uint64_t nbits) {
  const uint64_t nbytes = (nbits + 7) / 8;
  std::memcpy(out, words, nbytes);  // little-endian words == LSB-first bytes
  if (nbits & 7) out[nbytes - 1] &= (uint8_t)((1u << (nbits & 7)) - 1);
}

inline int pipe_chunks_cap() {
  const char* e = std::getenv("NT_PIPE_CHUNKS");
  const int v = e ? std::atoi(e) : kMaxChunks;
  return std::max(1, std::min(kMaxChunks, v));
}

// NT_PIPE_ROUND overrides the round size (tests use it to split small inputs)
inline uint64_t pipe_round(uint64_t R) {
  const char* e = std::getenv("NT_PIPE_ROUND");
  if (!e) return R;
  const uint64_t v = (uint64_t)std::max(64ll, std::atoll(e));
  return (v + 63) / 64 * 64;
}

// NT_PIPE_PLAN=round restores round 4's chunk plan (A/B; pipe_plan.hpp)
inline bool pipe_plan_round4() {
  static const bool r4 = [] {
    const char* e = std::getenv("NT_PIPE_PLAN");
    return e && std::strcmp(e, "round") == 0;
  }();
  return r4;
}
// chunk sizes of `total` items at round R (R a multiple of 64, so every boundary
// is too: each chunk owns whole 64-bit verdict words)
inline std::vector<uint64_t> chunk_targets(uint64_t total, uint64_t R) {
  return nt::chunk_targets(total, R, (uint64_t)pipe_chunks_cap(), pipe_plan_round4());
}
inline std::vector<uint64_t> verify_chunk_targets(uint64_t total, uint64_t R1) {
  return nt::verify_chunk_targets(total, R1, (uint64_t)pipe_chunks_cap());
}

// fn(lo, hi) over [0, n) in T = min(16, 1 + n / 16384) contiguous shares, on the
// host lane's pool threads above 16k items; the shares' results in order
template <class R, class F>
std::vector<R> pool_split(uint64_t n, F&& fn) {
  const uint64_t T = std::min<uint64_t>(16, 1 + n / 16384);
  std::vector<R> r(T);
  auto work = [&](uint64_t t) { r[t] = fn(n * t / T, n * (t + 1) / T); };
  if (T == 1) work(0);
  else nt::cpu::parallel_for_fn(T, (int)T, work);
  return r;
}

// Message bytes of items [lo, hi): the device buffer mirrors the host span
// [base, base + span) (16-B phase kept); chunk c copies just the bytes its items
// use, unless the items are not laid out in order, in which case chunk 0 copies
// the whole span once.
struct MsgStage {
  uint64_t base = 0, span = 0;
  bool whole = false;
  Chunks piece;  // per chunk [mn, mx), host-absolute
};

inline int msg_prepare(Device& dv, const uint64_t* off, const uint64_t* len, uint64_t lo, const Chunks& ch,
                       MsgStage& ms) {
  uint64_t gmn = UINT64_MAX, gmx = 0, sum = 0;
  ms.piece.clear();
  for (const auto& c : ch) {
    uint64_t mn = UINT64_MAX, mx = 0;
    for (uint64_t i = lo + c.first; i < lo + c.second; ++i) {
      if (len[i] == 0) continue;
      mn = std::min(mn, off[i]);
      mx = std::max(mx, off[i] + len[i]);
    }
    if (mn == UINT64_MAX) mn = mx = 0;
    ms.piece.emplace_back(mn, mx);
    sum += mx - mn;
    if (mx > mn) {
      gmn = std::min(gmn, mn);
      gmx = std::max(gmx, mx);
    }
  }
  if (gmn == UINT64_MAX) gmn = gmx = 0;
  ms.base = gmn & ~(uint64_t)15;
  ms.span = gmx - ms.base;
  ms.whole = sum > ms.span + ms.span / 4 + 4096;
  const uint64_t m = ch.back().second;
  NT_CHK(dv.d[B_DATA].ensure(ms.span + 64));
  NT_CHK(dv.d[B_OFF].ensure(std::max<uint64_t>(m, 1) * 16));
  NT_CHK(dv.h[B_OFF].ensure(std::max<uint64_t>(m, 1) * 16));
  return NT_OK;
}

// Device offsets / lengths of chunk [a, b) staged by msg_copy: words [2a, 2b) of
// B_OFF hold the chunk's b - a rebased offsets, then its b - a lengths (one copy)
inline const uint64_t* chunk_off(Device& dv, uint64_t a) { return dv.d[B_OFF].as<uint64_t>() + 2 * a; }
inline const uint64_t* chunk_len(Device& dv, uint64_t a, uint64_t b) {
  return dv.d[B_OFF].as<uint64_t>() + 2 * a + (b - a);
}

// copies (copy stream) of chunk c = items [lo + a, lo + b): rebased offsets,
// lengths, and the chunk's message bytes
inline int msg_copy(Device& dv, const uint8_t* data, const uint64_t* off, const uint64_t* len, uint64_t lo,
                    const MsgStage& ms, size_t c, uint64_t a, uint64_t b) {
  uint64_t* ho = dv.h[B_OFF].as<uint64_t>() + 2 * a;
  uint64_t* hl = ho + (b - a);
  for (uint64_t i = a; i < b; ++i) {
    ho[i - a] = len[lo + i] ? off[lo + i] - ms.base : 0;
    hl[i - a] = len[lo + i];
  }
  const auto& pc = ms.piece[c];
  if (ms.whole) {
    if (c == 0 && ms.span)
      NT_TRY(hipMemcpyAsync(dv.d[B_DATA].p, data + ms.base, ms.span, hipMemcpyHostToDevice, dv.cstream));
  } else if (pc.second > pc.first) {
    NT_TRY(hipMemcpyAsync(dv.d[B_DATA].as<uint8_t>() + (pc.first - ms.base), data + pc.first, pc.second - pc.first,
                          hipMemcpyHostToDevice, dv.cstream));
  }
  if (b > a)
    NT_TRY(hipMemcpyAsync(dv.d[B_OFF].as<uint64_t>() + 2 * a, ho, (b - a) * 16, hipMemcpyHostToDevice, dv.cstream));
  return NT_OK;
}

// every message byte a staged call copies lies in nt_host_alloc memory
inline bool ms_pinned(const MsgStage& ms, const uint8_t* data) {
  if (ms.span == 0) return true;
  if (ms.whole) return is_pinned(data + ms.base, ms.span);
  for (const auto& pc : ms.piece)
    if (pc.second > pc.first && !is_pinned(data + pc.first, pc.second - pc.first)) return false;
  return true;
}

// NT_PIPE_TRACE=1: host timestamps of every step of run_chunks on stderr (diagnosis)
inline bool pipe_trace() {
  static const bool on = [] {
    const char* e = std::getenv("NT_PIPE_TRACE");
    return e && *e == '1';
  }();
  return on;
}
inline double pipe_now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The chunk pipeline of a host entry point: copies(c) on the copy stream, then
// kernels(c) on compute stream cstr(c), launched by the host once it has waited
// for chunk c's copies -- a compute stream never holds a wait for the copy
// stream (a cross-queue wait pending at the head of a hardware queue slows the
// dispatches of the other queues: profiles/r05/ab_join.txt).  With every source
// in pinned memory (`async`) hipMemcpyAsync returns at once, and the copies of
// chunk c + 1 are queued before the host waits for chunk c, so the link never
// idles.  From pageable memory HIP stages the copy and returns when it is done
// (NT_PIPE_TRACE, profiles/r05/host_pipe_*.txt): then chunk c's kernels are
// launched before the copies of chunk c + 1 are issued, so they run under them.
// Returns with every kernel launched; finish_chunks() then waits for both
// compute streams on the host.
template <class Copy, class Launch>
int run_chunks(Device& dv, size_t C, bool async, Copy&& copy, Launch&& launch) {
  if (C == 0) return NT_OK;
  if (C > (size_t)kMaxChunks) return NT_EINVAL;
  const bool tr = pipe_trace();
  const double t0 = tr ? pipe_now_us() : 0.0;
  auto issue = [&](size_t c) -> int {
    NT_CHK(copy(c));
    NT_TRY(hipEventRecord(dv.cev[c], dv.cstream));
    if (tr) std::fprintf(stderr, "[pipe] %9.1f copies %zu issued%s\n", pipe_now_us() - t0, c, async ? "" : " (staged)");
    return NT_OK;
  };
  if (async) NT_CHK(issue(0));
  for (size_t c = 0; c < C; ++c) {
    if (!async) NT_CHK(issue(c));
    else if (c + 1 < C) NT_CHK(issue(c + 1));
    NT_TRY(hipEventSynchronize(dv.cev[c]));
    if (tr) std::fprintf(stderr, "[pipe] %9.1f copies %zu done\n", pipe_now_us() - t0, c);
    NT_CHK(launch(c));
    if (tr) std::fprintf(stderr, "[pipe] %9.1f kernels %zu launched\n", pipe_now_us() - t0, c);
  }
  return NT_OK;
}

// run_chunks for sources that need host staging (a memcpy into the pinned
// buffers before the DMA): a helper thread stages and issues the copies of every
// chunk in order, running ahead of the launches, while this thread waits for each
// chunk's copies and launches its kernels -- the staging of chunk c+1 overlaps
// both chunk c's DMA and its kernels, and no launch waits behind a memcpy.  The
// copy callbacks run on the helper thread only (they must not share mutable
// state with the launch callbacks).
template <class Copy, class Launch>
int run_chunks_staged(Device& dv, size_t C, Copy&& copy, Launch&& launch) {
  if (C <= 1) return run_chunks(dv, C, false, copy, launch);
  if (C > (size_t)kMaxChunks) return NT_EINVAL;
  const bool tr = pipe_trace();
  const double t0 = tr ? pipe_now_us() : 0.0;
  int hip_dev = 0;
  NT_TRY(hipGetDevice(&hip_dev));
  std::mutex mu;
  std::condition_variable cv;
  size_t issued = 0;
  int err = NT_OK;
  std::thread helper([&] {
    int rc = hipSetDevice(hip_dev) == hipSuccess ? NT_OK : NT_EHIP;
    for (size_t c = 0; c < C && rc == NT_OK; ++c) {
      rc = copy(c);
      if (rc == NT_OK && hipEventRecord(dv.cev[c], dv.cstream) != hipSuccess) rc = NT_EHIP;
      if (tr && rc == NT_OK) std::fprintf(stderr, "[pipe] %9.1f copies %zu staged+issued\n", pipe_now_us() - t0, c);
      std::lock_guard<std::mutex> lk(mu);
      if (rc == NT_OK) ++issued;
      else err = rc;
      cv.notify_one();
    }
  });
  int rc = NT_OK;
  for (size_t c = 0; c < C && rc == NT_OK; ++c) {
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return issued > c || err != NT_OK; });
      if (issued <= c) break;  // the helper failed before issuing chunk c
    }
    if (hipEventSynchronize(dv.cev[c]) != hipSuccess) {
      rc = NT_EHIP;
      break;
    }
    if (tr) std::fprintf(stderr, "[pipe] %9.1f copies %zu done\n", pipe_now_us() - t0, c);
    rc = launch(c);
    if (tr) std::fprintf(stderr, "[pipe] %9.1f kernels %zu launched\n", pipe_now_us() - t0, c);
  }
  helper.join();
  return rc != NT_OK ? rc : err;
}

// Per-chunk host work that runs on a thread of its own, chunk by chunk ahead of
// run_chunks_staged's copy callbacks: step(c) for c = 0 .. C - 1 in order;
// wait(c) returns once step(c) is done.  A copy callback issues what does not
// depend on the step, then waits, so a pageable copy of chunk c (HIP stages it
// and returns when it is done) overlaps step(c + 1).  The destructor stops
// after the step in flight and joins.
class LookAhead {
 public:
  template <class Step>
  void start(size_t C, Step step) {
    th_ = std::thread([this, C, step] {
      for (size_t c = 0; c < C && !stop_; ++c) {
        step(c);
        std::lock_guard<std::mutex> lk(mu_);
        ready_ = c + 1;
        cv_.notify_all();
      }
    });
  }
  void wait(size_t c) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return ready_ > c; });
  }
  void join() {
    if (th_.joinable()) th_.join();
  }
  ~LookAhead() {
    stop_ = true;
    join();
  }

 private:
  std::thread th_;
  std::mutex mu_;
  std::condition_variable cv_;
  size_t ready_ = 0;
  std::atomic<bool> stop_{false};
};

// both compute streams drained (host-side), so work issued next on lane 0's stream
// follows every chunk's kernels without a cross-queue wait
inline int finish_chunks(Device& dv) {
  if (dv.lane[1].stream != dv.lane[0].stream) NT_TRY(hipStreamSynchronize(dv.lane[1].stream));
  return NT_OK;
}

}  // namespace ntrt
