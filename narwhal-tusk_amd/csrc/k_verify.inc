// k_verify.inc -- the general verification kernel (NPER = two signatures per
// lane, or one for the host entry points' short chunks; half-size scalars) and
// its per-mode launcher; included by k_verify_<mode>_b<width>.hip.
#include "kernels_common.hpp"

namespace nt {

// --------------------------------------------------------------------------
// Verification: NPER signatures per lane, grid-stride over workspace slots.
// Block iteration covers NPER x 256 signatures; wave w, lane l, slot j handles
// signature base + 64 NPER w + 64 j + l (so each verdict word is one ballot).
// NPER = 1 halves the per-lane latency of a launch (a lane's signatures run one
// after the other): the host entry points' last chunk, whose kernel is all
// that is left after the last PCIe copy (DESIGN.md §6.4).
// --------------------------------------------------------------------------
// KTAB: the variant that carries the key-table cache (DevKTab).  A launch without a cache
// (none allocated, NT_KTAB_KEYS=0, or an occupancy other than the default's) runs the KTAB =
// false variant, whose code is the kernel's as it was before the cache: nothing of the cache is
// compiled beside its balanced path.
template <int MODE, int OCC, int WB, int NPER, bool KTAB>
__global__ __launch_bounds__(kBlock, OCC) void k_ed25519_verify(
    const uint32_t* __restrict__ pk, const uint32_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint64_t msg_bytes, const uint64_t* __restrict__ off, const uint64_t* __restrict__ len, uint64_t n,
    const uint32_t* __restrict__ combB, uint4* __restrict__ ws, unsigned long long* __restrict__ out_bits,
    uint4* xtab, uint32_t xmask, uint32_t* kbase, uint32_t kcap) {
  WsATab at{ws, blockIdx.x};
  const WideComb<WB> wb{combB};
  const DevXCache xc{xtab, xmask};
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wofs = 64 * NPER * (uint64_t)(threadIdx.x >> 6);
  for (uint64_t base = (uint64_t)blockIdx.x * NPER * kBlock; base < n;
       base += (uint64_t)gridDim.x * NPER * kBlock) {
    uint32_t act[NPER];
    const uint32_t* A[NPER];
    const uint32_t* S[NPER];
    const uint8_t* M[NPER];
    uint64_t L[NPER];
#pragma unroll
    for (int j = 0; j < NPER; ++j) {
      const uint64_t gi = base + wofs + 64 * j + lane;
      const uint64_t i = gi < n ? gi : n - 1;
      const MsgSlice ms = msg_slice(off[i], len[i], msg_bytes);  // out of bounds: rejected
      act[j] = (gi < n) & ms.ok;
      A[j] = pk + 8 * i;
      S[j] = sig + 16 * i;
      M[j] = msg + ms.off;
      L[j] = ms.len;
    }
    uint32_t ok[NPER];
    if constexpr (KTAB) {
      const DevKTab kt{kbase, kcap};
      // act: lanes past n (they repeat entry n - 1) and lanes with a bad slice leave the cache alone
      verify_n<MODE, NPER>(ok, A, S, M, L, at, wb, xc, kt, act);
    } else {
      verify_n<MODE, NPER>(ok, A, S, M, L, at, wb, xc);
    }
#pragma unroll
    for (int j = 0; j < NPER; ++j) {
      const unsigned long long bal = __ballot(ok[j] & act[j]);
      const uint64_t wbase = base + wofs + 64 * j;
      if (lane == 0 && wbase < n) out_bits[wbase >> 6] = bal;
    }
  }
}

// per_lane: 1 or kVPer signatures per lane (blocks = verify_grid(n, slots, per_lane));
// one signature per lane is built for the default occupancy only
template <int MODE, int WB>
hipError_t launch_verify_m(uint64_t blocks, const uint8_t* d_pk, const uint8_t* d_sig, const uint8_t* d_msg,
                           uint64_t msg_bytes, const uint64_t* d_off, const uint64_t* d_len, uint64_t n,
                           const uint32_t* d_combB, void* d_ws, uint64_t* d_out_words, hipStream_t s, int per_lane,
                           XTab xt, KTabArgs kt) {
  const int occ = verify_occupancy();
#define NT_V_LAUNCH(O, P) NT_V_LAUNCH_K(O, P, false)
#define NT_V_LAUNCH_K(O, P, K)                                                                             \
  hipLaunchKernelGGL((k_ed25519_verify<MODE, O, WB, P, K>), dim3((uint32_t)blocks), dim3(kBlock), 0, s,       \
                     (const uint32_t*)d_pk, (const uint32_t*)d_sig, d_msg, msg_bytes, d_off, d_len, n, d_combB, \
                     (uint4*)d_ws, (unsigned long long*)d_out_words, (uint4*)xt.tab, xt.mask,                   \
                     (uint32_t*)kt.base, kt.cap)
  if (per_lane == 1 && kVPer != 1) {
    if (occ != 2) return hipErrorInvalidValue;  // verify_per_lane_for() never asks for it
    if (kt.base) NT_V_LAUNCH_K(2, 1, true);
    else NT_V_LAUNCH(2, 1);
  } else if (occ == 1) {
    NT_V_LAUNCH(1, kVPer);
  } else if (occ == 3) {
    NT_V_LAUNCH(3, kVPer);
  } else if (kt.base) {
    NT_V_LAUNCH_K(2, kVPer, true);
  } else {
    NT_V_LAUNCH(2, kVPer);
  }
#undef NT_V_LAUNCH_K
#undef NT_V_LAUNCH
  return hipGetLastError();
}

}  // namespace nt
