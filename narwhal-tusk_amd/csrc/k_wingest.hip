// k_wingest.hip -- the worker's message ingestion on the device: bincode
// WorkerMessage bytes, copied to HBM as they arrived from another worker
// (worker/src/worker.rs:270-292), are told apart, validated and measured
// without a host decode; the SHA-512 launch that follows gives an accepted
// batch the digest the Processor computes (worker/src/processor.rs:38).
//
//   k_wmsg_walk     one wave per message: the layout of wmsg_plan.hpp.  A batch's
//                   length-prefixed transactions are a pointer chase, walked 64
//                   at a time by proven speculation (wmsg_round_*: each lane reads
//                   the prefix its position would have if the next transactions
//                   all had the hypothesised length, a ballot finds the leading
//                   run that is proven); a request's 44 key characters are
//                   decoded one per lane.  Writes the code, the receipt's rows
//                   (a batch's digest still zero) and the length the SHA-512
//                   launch is to hash: the whole message for an accepted batch,
//                   0 for everything else.
//   k_wmsg_receipt  one thread per message, only when the call asked for
//                   receipts: the 64-byte record with an accepted batch's digest
//                   put in, written as four 16-byte stores.
// Message bytes are read with aligned dword loads joined by v_alignbyte (the
// wire buffer keeps 64 bytes of slack on both sides), so messages may start at
// any byte.  No LDS, no atomics, no scratch.
#include "kernels_common.hpp"
#include "wingest.hpp"
#include "wmsg_plan.hpp"

namespace nt {

namespace {

constexpr int kWavesPerBlock = kBlock / 64;

// the helpers of k_ingest.hip (kept there too: that unit's device code stays as it is)
NT_D NT_INLINE uint32_t ldu32(const uint8_t* p) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
  return __builtin_amdgcn_alignbyte(q[1], q[0], (uint32_t)(a & 3));
}
NT_D NT_INLINE uint64_t ldu64(const uint8_t* p) { return ldu32(p) | ((uint64_t)ldu32(p + 4) << 32); }
NT_D NT_INLINE uint32_t ldu8(const uint8_t* p) {
  const uintptr_t a = (uintptr_t)p;
  return (*(const uint32_t*)(a & ~(uintptr_t)3) >> (8 * (uint32_t)(a & 3))) & 0xffu;
}
// wmsg_plan.hpp's loader over the wire bytes of one message
struct WireLd {
  const uint8_t* p;
  NT_D NT_INLINE uint32_t u8(uint64_t o) const { return ldu8(p + o); }
  NT_D NT_INLINE uint32_t u32(uint64_t o) const { return ldu32(p + o); }
  NT_D NT_INLINE uint64_t u64(uint64_t o) const { return ldu64(p + o); }
};

// lane k's value (k the same in every lane)
NT_D NT_INLINE uint32_t lane32(uint32_t x, uint32_t k) {
  return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)__builtin_amdgcn_readfirstlane((int)k));
}
NT_D NT_INLINE uint64_t lane64(uint64_t x, uint32_t k) {
  return lane32((uint32_t)x, k) | ((uint64_t)lane32((uint32_t)(x >> 32), k) << 32);
}

}  // namespace

__global__ __launch_bounds__(kBlock) void k_wmsg_walk(WmsgBufs b) {
  aux_priority();
  const uint64_t i = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (i >= b.n) return;  // whole waves
  // a message outside the chunk's bytes is an empty one: never read
  const MsgSlice ms = msg_slice(b.moff[i], b.mlen[i], b.wire_bytes);
  const uint8_t* p = b.wire + ms.off;
  const uint64_t L = ms.len;
  // every value below but q, v, valid, c and dig is the same in all lanes
  const WireLd ld{p};
  WmsgPlan m = wmsg_head(ld, L);
  uint32_t dig = 0;  // lane 8 + j: word j of a request's raw key
  if (m.code == kWmsgOk && m.kind == kWmsgRequest) {
    const uint32_t t = lane < kWmsgKeyChars ? lane : (uint32_t)kWmsgKeyChars - 1;
    const uint32_t c = ldu8(p + m.off_key + t);
    if (__ballot(!wmsg_b64_char_ok(t, c)) != 0) {
      m = wmsg_fail(kWmsgHost);
    } else {
      const uint32_t v = wmsg_b64_val(c);
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t by = 4 * (lane & 7u) + k, t0 = wmsg_b64_first_char(by);
        dig |= wmsg_b64_byte(by, (uint32_t)__shfl((int)v, (int)t0), (uint32_t)__shfl((int)v, (int)t0 + 1)) << (8 * k);
      }
    }
  } else if (m.code == kWmsgOk) {
    WmsgWalk w = wmsg_walk_start(m);
    while (w.r) {
      uint64_t q;
      const bool valid = wmsg_lane_at(w, L, lane, &q);
      const uint64_t v = valid ? ldu64(p + q) : 0;
      const uint64_t s = lane64(v, 0);
      const uint64_t agree = __ballot(wmsg_lane_agrees(w, L, lane, valid, q, v, s));
      const uint64_t na = ~agree;
      const uint32_t k = na ? (uint32_t)__builtin_ctzll(na) : 0u;
      wmsg_round_end(w, lane32(valid, 0) != 0, s, agree, lane32(valid, k) != 0, lane64(v, k));
    }
    m = wmsg_batch_done(m, w);
  }
  uint32_t* out = (uint32_t*)(b.plan + 4 * i);
  if (lane == 0) {
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t w[kWmsgReceiptWords];
    wmsg_receipt_words(m, zero, w);
    b.plan[4 * i] = make_uint4(w[0], w[1], w[2], w[3]);
    b.plan[4 * i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
    b.hlen[i] = m.code == kWmsgOk && m.kind == kWmsgBatch ? L : 0;
    b.code[i] = (uint8_t)m.code;
  } else if (lane >= 8 && lane < 16) {
    out[lane] = m.code == kWmsgOk ? dig : 0u;
  }
}

// The receipt of message i: the rows k_wmsg_walk wrote, with the digest of the SHA-512
// launch in an accepted batch's (every other message was hashed as an empty one: unused).
__global__ __launch_bounds__(kBlock) void k_wmsg_receipt(WmsgBufs b) {
  aux_priority();
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= b.n) return;
  // native vectors: a uint4 assigned under a condition becomes a private array, which the
  // compiler then moves to LDS
  typedef uint32_t u4v __attribute__((ext_vector_type(4)));
  const u4v* row = (const u4v*)(b.plan + 4 * i);
  const u4v r0 = row[0], r1 = row[1];
  const bool batch = (r0.x & 0xffffu) == (kWmsgOk | (kWmsgBatch << 8));
  const u4v* d = batch ? (const u4v*)(b.sha + 32 * i) : row + 2;
  const u4v r2 = d[0], r3 = d[1];
  u4v* out = (u4v*)(b.rec + 4 * i);
  out[0] = r0;
  out[1] = r1;
  out[2] = r2;
  out[3] = r3;
}

hipError_t launch_wmsg_walk(const WmsgBufs& b, hipStream_t s) {
  if (b.n == 0) return hipSuccess;
  const uint64_t blocks = (b.n + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL(k_wmsg_walk, dim3((uint32_t)blocks), dim3(kBlock), 0, s, b);
  return hipGetLastError();
}
hipError_t launch_wmsg_receipt(const WmsgBufs& b, hipStream_t s) {
  if (b.n == 0) return hipSuccess;
  if (!b.rec || !b.sha) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_wmsg_receipt, dim3((uint32_t)((b.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, b);
  return hipGetLastError();
}

}  // namespace nt
