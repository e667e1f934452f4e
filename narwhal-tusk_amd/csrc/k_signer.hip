// k_signer.hip -- gfx950 kernels of a signer bound to the node's own key (signer_ops.hpp),
// instantiated for both widths of the comb of B like k_ed25519_sign:
//
//   k_signer_votes<WB>    one vote per lane: Vote::digest, its signature and the 212 bytes of
//                         PrimaryMessage::Vote (primary/src/core.rs:184-211, messages.rs:114-129);
//                         a wave assembles its row of 64 records in LDS and writes it as
//                         contiguous 16-byte stores
//   k_signer_digests<WB>  SignatureService::request_signature for n 32-byte digests
//                         (crypto/src/lib.rs:229-250)
//
// NOT CONSTANT TIME (signer_ops.hpp): comb lookups by digits of the nonce, a variable-time inversion.
#include "kernels_common.hpp"
#include "signer_ops.hpp"

namespace nt {

constexpr int kSignerRow = 64;                                 // votes per wave iteration = one workgroup
constexpr int kSignerRowBytes = kSignerRow * kVoteWireBytes;   // 13,568 = 848 x 16
constexpr int kSignerRowQuads = kSignerRowBytes / 16;
static_assert(kSignerRowQuads * 16 == kSignerRowBytes, "a row of votes is whole 16-byte stores");

// the key record, read once per wave (every lane the same address)
NT_D NT_INLINE void signer_key_load(SignerKey& k, const uint32_t* __restrict__ p) {
  uint32_t* w = (uint32_t*)&k;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(SignerKey) / 4); ++i) w[i] = p[i];
}

template <int WB>
__global__ __launch_bounds__(kSignerRow) void k_signer_votes(const uint32_t* __restrict__ keyrec,
                                                            const uint32_t* __restrict__ id,
                                                            const uint64_t* __restrict__ round,
                                                            const uint32_t* __restrict__ origin, uint64_t n,
                                                            const uint32_t* __restrict__ combB,
                                                            uint32_t* __restrict__ out_vote,
                                                            uint32_t* __restrict__ out_digest) {
  __shared__ __attribute__((aligned(16))) uint32_t s_row[kSignerRow * kVoteWireWords];
  const WideComb<WB> wb{combB};
  SignerKey key;
  signer_key_load(key, keyrec);
  const uint32_t lane = threadIdx.x;
  for (uint64_t base = (uint64_t)blockIdx.x * kSignerRow; base < n; base += (uint64_t)gridDim.x * kSignerRow) {
    const uint64_t gi = base + lane;
    const uint32_t active = gi < n;
    const uint64_t i = active ? gi : n - 1;  // lanes past n repeat the last entry and store nothing
    uint32_t idw[8], ow[8];
    ld8(idw, id + 8 * i);
    ld8(ow, origin + 8 * i);
    const uint64_t rd = round[i];
    uint32_t rec[kVoteWireWords], dg[8];
    vote_one(rec, dg, key, idw, rd, ow, wb);
    if (active && out_digest) {
      uint4* po = (uint4*)(out_digest + 8 * i);
      po[0] = make_uint4(dg[0], dg[1], dg[2], dg[3]);
      po[1] = make_uint4(dg[4], dg[5], dg[6], dg[7]);
    }
    // the row in LDS, record-major: lane l's dword j at 53 l + j (an odd stride: no bank conflicts)
#pragma unroll
    for (int j = 0; j < kVoteWireWords; ++j) s_row[lane * kVoteWireWords + j] = rec[j];
    __syncthreads();
    // ... and out as one contiguous run: the row starts at byte 13,568 (base / 64) of the array.
    // The last row of a launch writes only its (n - base) x 212 bytes: whole 16-byte stores, then dwords.
    const uint64_t left = n - base;
    const uint32_t bytes = left >= (uint64_t)kSignerRow ? (uint32_t)kSignerRowBytes : (uint32_t)left * kVoteWireBytes;
    const uint32_t quads = bytes >> 4, tail = (bytes & 15u) >> 2;
    uint32_t* dst = out_vote + base * kVoteWireWords;
#pragma unroll 1
    for (uint32_t t = lane; t < quads; t += kSignerRow) ((uint4*)dst)[t] = ((const uint4*)s_row)[t];
    if (lane < tail) dst[4 * quads + lane] = s_row[4 * quads + lane];
    __syncthreads();
  }
}

template <int WB>
__global__ __launch_bounds__(kBlock) void k_signer_digests(const uint32_t* __restrict__ keyrec,
                                                          const uint32_t* __restrict__ digest, uint64_t n,
                                                          const uint32_t* __restrict__ combB,
                                                          uint32_t* __restrict__ out_sig) {
  const WideComb<WB> wb{combB};
  SignerKey key;
  signer_key_load(key, keyrec);
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t gi = base + threadIdx.x;
    const uint32_t active = gi < n;
    const uint64_t i = active ? gi : n - 1;
    uint32_t m[8], Rw[8], s[8];
    ld8(m, digest + 8 * i);
    sign_fixed_one(Rw, s, key, m, wb);
    if (active) {
      uint4* so = (uint4*)(out_sig + 16 * i);
      so[0] = make_uint4(Rw[0], Rw[1], Rw[2], Rw[3]);
      so[1] = make_uint4(Rw[4], Rw[5], Rw[6], Rw[7]);
      so[2] = make_uint4(s[0], s[1], s[2], s[3]);
      so[3] = make_uint4(s[4], s[5], s[6], s[7]);
    }
  }
}

// The device arrays are 16-byte aligned (id, origin, digest, the outputs) and round 8-byte
// aligned: the host runtime's buffers are, and nts_dev_votes_sign refuses others.
hipError_t launch_signer_votes(const void* d_key, const uint8_t* d_id, const uint64_t* d_round, const uint8_t* d_origin,
                               uint64_t n, const uint32_t* d_combB, int bbits, uint8_t* d_vote, uint8_t* d_digest,
                               uint32_t max_rows, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!d_combB || !d_key) return hipErrorInvalidValue;
  uint64_t blocks = (n + kSignerRow - 1) / kSignerRow;
  if (blocks > max_rows) blocks = max_rows;
#define NT_SIGNER_LAUNCH(WB)                                                                            \
  hipLaunchKernelGGL(k_signer_votes<WB>, dim3((uint32_t)blocks), dim3(kSignerRow), 0, s,               \
                     (const uint32_t*)d_key, (const uint32_t*)d_id, d_round, (const uint32_t*)d_origin, n, d_combB, \
                     (uint32_t*)d_vote, (uint32_t*)d_digest)
  if (bbits == kBCombBits) NT_SIGNER_LAUNCH(kBCombBits);
  else if (bbits == kBCombFallback) NT_SIGNER_LAUNCH(kBCombFallback);
  else return hipErrorInvalidValue;
#undef NT_SIGNER_LAUNCH
  return hipGetLastError();
}

hipError_t launch_signer_digests(const void* d_key, const uint8_t* d_digest, uint64_t n, const uint32_t* d_combB,
                                 int bbits, uint8_t* d_sig, uint32_t max_blocks, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!d_combB || !d_key) return hipErrorInvalidValue;
  uint64_t blocks = (n + kBlock - 1) / kBlock;
  if (blocks > max_blocks) blocks = max_blocks;
#define NT_SIGNER_LAUNCH(WB)                                                                   \
  hipLaunchKernelGGL(k_signer_digests<WB>, dim3((uint32_t)blocks), dim3(kBlock), 0, s,        \
                     (const uint32_t*)d_key, (const uint32_t*)d_digest, n, d_combB, (uint32_t*)d_sig)
  if (bbits == kBCombBits) NT_SIGNER_LAUNCH(kBCombBits);
  else if (bbits == kBCombFallback) NT_SIGNER_LAUNCH(kBCombFallback);
  else return hipErrorInvalidValue;
#undef NT_SIGNER_LAUNCH
  return hipGetLastError();
}

}  // namespace nt
