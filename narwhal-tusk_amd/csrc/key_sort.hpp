// key_sort.hpp -- the counting sort behind the key-grouped order of key-cache
// launches (k_misc.hip launch_verify_keyset): slot -> signature, grouped by
// committee index.  A header of its own so that the device probe
// (tests/cpp/nt_device_probe.hip) launches the same two kernels with the same
// geometry and reads the permutation back: the key-cache kernel loads every
// signature's key by the signature's own index, so its verdicts cannot show
// whether the slots are grouped at all.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_common.hpp"

namespace nt {

constexpr uint32_t kSortBuckets = 4096;  // committee keys + 1 "unknown" bucket
constexpr uint64_t kSortMin = 65536;     // smaller launches keep the input order
constexpr int kSortTile = 16;            // items per thread of k_key_scatter
constexpr int kHistTile = 16;            // independent key loads in flight per thread of k_key_hist
// Global bucket counters one 128-B line apart: every block's flush / reservation
// is one device-scope atomic per bucket, and with the counters packed 32 to a
// line those atomics serialize per LINE (rocprof r03b: k_key_scatter 66 us at
// 1,661 blocks, ~1.6 ns per atomic on one of 4 lines; k_key_hist 43 us whatever
// the size, one dependent load + LDS atomic per loop iteration).
constexpr uint32_t kCtrStride = 32;

NT_D NT_INLINE uint32_t sort_bucket(uint32_t k, int mixed, uint32_t nkeys) {
  if (mixed) k &= ~kKeyWantStrict;
  return k < nkeys ? k : nkeys;
}

static __global__ __launch_bounds__(kBlock) void k_key_hist(const uint32_t* __restrict__ key, uint64_t n, int mixed,
                                                    uint32_t nkeys, uint32_t* __restrict__ hist) {
  aux_priority();
  extern __shared__ uint32_t sort_lds[];  // nkeys + 1 counters (launch_verify_keyset sizes it)
  uint32_t* h = sort_lds;
  for (uint32_t b = threadIdx.x; b <= nkeys; b += kBlock) h[b] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * kBlock * kHistTile;
  for (uint64_t t0 = (uint64_t)blockIdx.x * kBlock * kHistTile; t0 < n; t0 += stride) {
    uint32_t k[kHistTile];
#pragma unroll
    for (int r = 0; r < kHistTile; ++r) {  // all loads issued before the first is used
      const uint64_t i = t0 + (uint64_t)r * kBlock + threadIdx.x;
      k[r] = i < n ? key[i] : 0u;
    }
#pragma unroll
    for (int r = 0; r < kHistTile; ++r)
      if (t0 + (uint64_t)r * kBlock + threadIdx.x < n) atomicAdd(&h[sort_bucket(k[r], mixed, nkeys)], 1u);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b <= nkeys; b += kBlock)
    if (h[b]) atomicAdd(&hist[b * kCtrStride], h[b]);
}

// Each block computes the exclusive prefix of the global histogram itself (the
// counts are final: k_key_hist ran before on the stream) and reserves its
// ranges with one atomic per bucket on the bucket line's second word (zeroed
// with the histogram by one memset): no separate scan launch.
static __global__ __launch_bounds__(kBlock) void k_key_scatter(const uint32_t* __restrict__ key, uint64_t n, int mixed,
                                                       uint32_t nkeys, uint32_t* __restrict__ lines,
                                                       uint32_t* __restrict__ perm) {
  aux_priority();
  extern __shared__ uint32_t sort_lds[];  // cnt[nkeys + 1], base[nkeys + 1], part[kBlock]
  const uint32_t nb = nkeys + 1;
  uint32_t* cnt = sort_lds;
  uint32_t* base = sort_lds + nb;
  uint32_t* part = sort_lds + 2 * nb;
  const uint32_t per = (nb + kBlock - 1) / kBlock, b0 = threadIdx.x * per;
  uint32_t sum = 0;
  for (uint32_t b = b0; b < b0 + per && b < nb; ++b) sum += lines[b * kCtrStride];
  part[threadIdx.x] = sum;
  for (uint32_t b = threadIdx.x; b <= nkeys; b += kBlock) cnt[b] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (int t = 0; t < kBlock; ++t) {
      const uint32_t v = part[t];
      part[t] = acc;
      acc += v;
    }
  }
  __syncthreads();
  {
    uint32_t acc = part[threadIdx.x];
    for (uint32_t b = b0; b < b0 + per && b < nb; ++b) {
      base[b] = acc;
      acc += lines[b * kCtrStride];
    }
  }
  const uint64_t t0 = (uint64_t)blockIdx.x * kBlock * kSortTile;
  uint32_t bk[kSortTile], rk[kSortTile];
#pragma unroll
  for (int r = 0; r < kSortTile; ++r) {
    const uint64_t i = t0 + (uint64_t)r * kBlock + threadIdx.x;
    bk[r] = i < n ? sort_bucket(key[i], mixed, nkeys) : 0u;
    rk[r] = i < n ? atomicAdd(&cnt[bk[r]], 1u) : 0u;
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b <= nkeys; b += kBlock)
    if (cnt[b]) base[b] += atomicAdd(&lines[b * kCtrStride + 1], cnt[b]);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortTile; ++r) {
    const uint64_t i = t0 + (uint64_t)r * kBlock + threadIdx.x;
    if (i < n) perm[base[bk[r]] + rk[r]] = (uint32_t)i;
  }
}

// perm[0 .. m) = the m signatures of d_key_idx grouped by bucket (committee index; every index
// >= nkeys, the strict bit of mixed mode aside, in bucket nkeys), on stream s.  `lines`: the
// nkeys + 1 bucket lines of kCtrStride words, zeroed by the caller (k_ks_init).
inline hipError_t launch_key_sort(const uint32_t* d_key_idx, uint64_t m, int mixed, uint32_t nkeys, uint32_t* lines,
                                  uint32_t* perm, hipStream_t s) {
  if (m == 0 || m > 0xFFFFFFFFull || nkeys + 1 > kSortBuckets) return hipErrorInvalidValue;
  // one tile of kHistTile keys per thread and at most 512 blocks (each flushes its
  // LDS histogram with one global atomic per bucket)
  const uint64_t hw = (m + (uint64_t)kBlock * kHistTile - 1) / ((uint64_t)kBlock * kHistTile);
  const uint32_t hb = (uint32_t)(hw < 512 ? hw : 512);
  // LDS sized to the committee (nkeys + 1 buckets), not to kSortBuckets: a
  // 101-key committee's scatter block takes 1.8 KB instead of 33 KB, so it
  // finds room on a CU beside the other stream's key-cache launch
  // (profiles/r06/shard8_trace_r06p.txt: the 33 KB blocks waited ~0.7 ms)
  const size_t hist_lds = 4ull * (nkeys + 1), scat_lds = 4ull * (2ull * (nkeys + 1) + kBlock);
  hipLaunchKernelGGL(k_key_hist, dim3(hb), dim3(kBlock), hist_lds, s, d_key_idx, m, mixed, nkeys, lines);
  const uint64_t sb = (m + (uint64_t)kBlock * kSortTile - 1) / ((uint64_t)kBlock * kSortTile);
  hipLaunchKernelGGL(k_key_scatter, dim3((uint32_t)sb), dim3(kBlock), scat_lds, s, d_key_idx, m, mixed, nkeys, lines,
                     perm);
  return hipGetLastError();
}

}  // namespace nt
