// wcomb_build.hpp -- wide-comb construction: the sizes of a comb and of the
// builders' scratch, one key's bases, the thread -> (key, position, chunk) map
// of the fill kernel and the offsets of a batch's launch, the two builder
// kernels and the launcher that batches them.
// Included by k_misc.hip (the product's launch_wcomb_build and size functions)
// and by tests/cpp/nt_device_probe.hip, which builds combs with the same
// launcher; the sizes and the thread map also compile for the host
// (tests/cpp/nt_host_harness.cpp), the kernels only under hipcc.
#pragma once
#include <stddef.h>

#include "ed25519_ops.hpp"

namespace nt {

// what: 0 bytes of a comb, 1 bytes of a key's bases, 2 bytes of a key's fill
// scratch (tmp), 3 keys per fill launch: >= 128k threads per launch (16 keys
// at W = 16, 2 at W = 20)
template <int W>
inline size_t comb_size(int what) {
  using G = CombGeom<W>;
  switch (what) {
    case 0: return G::kWordsPerPoint * 4;
    case 1: return (size_t)G::kPos * 40 * 4;
    case 2: return (size_t)G::kPos * G::kChunks * kWChunk * 10 * 4;
    default: {
      const uint64_t per_key = (uint64_t)G::kPos * G::kChunks, keys = (128u << 10) / per_key;
      return (size_t)(keys > 1 ? keys : 1);
    }
  }
}
inline size_t comb_size(int bits, int what) {
  return bits == kKeyCombReduced  ? comb_size<kKeyCombReduced>(what)
         : bits == kKeyCombWide   ? comb_size<kKeyCombWide>(what)
         : bits == kKeyCombMid    ? comb_size<kKeyCombMid>(what)
         : bits == kKeyCombNarrow ? comb_size<kKeyCombNarrow>(what)
         : bits == kBCombBits     ? comb_size<kBCombBits>(what)
                                  : 0;
}

// Thread t of a fill launch over nkeys keys: one thread per (key, position,
// chunk of 64 entries).  dst: word offset, from the launch's comb pointer, of
// the chunk's first entry (entry 1 + 64 chunk of the position; chunk 0 also
// writes entry 0, one entry before it); tmp: word offset of the thread's 640
// words of scratch.  Returns false, and leaves ft alone, for a thread past the
// launch's work.
struct WCombFillTarget {
  uint32_t key, pos, chunk;
  size_t dst, tmp;
};
template <int W>
NT_HD NT_INLINE bool wcomb_fill_target(WCombFillTarget& ft, uint64_t t, uint32_t nkeys) {
  using G = CombGeom<W>;
  const uint64_t per_key = (uint64_t)G::kPos * G::kChunks;
  if (t >= per_key * nkeys) return false;
  const uint32_t key = (uint32_t)(t / per_key);
  const uint32_t pos = (uint32_t)((t % per_key) / G::kChunks);
  const uint32_t c = (uint32_t)(t % G::kChunks);
  ft = WCombFillTarget{key, pos, c, key * G::kWordsPerPoint + ((size_t)pos * G::kEntries + 1 + (size_t)kWChunk * c) * kWStride,
                       (size_t)(t * (kWChunk * 10))};
  return true;
}

// One point of a build: decode (or take B), optionally negate, write the kPos
// bases 2^(W i) P to `bases` and the kKey* bits to *meta (unless null), which are
// also returned.  A key that does not decode
// gets identity bases (every entry the identity; such keys always reject via
// meta).  Reduced-scalar combs (CombGeom::kReduced) also get the point's [L]P
// entry (32 words at `corr`, which follows the positions) and kKeyTorsion when
// it is not the identity.
template <int W>
NT_HD NT_INLINE uint32_t wcomb_key_bases(const uint32_t w[8], int negate, uint32_t* bases, uint32_t* corr,
                                         uint32_t* meta) {
  ge_p3 P;
  const uint32_t ok = ge_frombytes_w(P, w);
  uint32_t m = (ok ? kKeyDecodes : 0u) | (ge_is_small_order(P) ? kKeySmallOrder : 0u);
  if (!ok) ge_p3_0(P);
  if (negate) {
    fe_neg(P.X, P.X);
    fe_carry(P.X);
    fe_neg(P.T, P.T);
    fe_carry(P.T);
  }
  if (CombGeom<W>::kReduced) {
    ge_niels q;
    m |= wcomb_corr(q, P) ? kKeyTorsion : 0u;
    uint32_t* o = corr;
#pragma unroll
    for (int l = 0; l < 10; ++l) { o[l] = q.ypx.v[l]; o[10 + l] = q.ymx.v[l]; o[20 + l] = q.xy2d.v[l]; }
    o[30] = 0;
    o[31] = 0;
  }
  if (meta) *meta = m;
  wcomb_bases<W>(bases, P);
  return m;
}

// The fill launch of the keys [k0, k0 + nkeys) of a build of `total` keys, at
// most `batch` per launch: its threads and the word offsets of its keys' bases
// and combs (the kernel numbers the launch's keys from 0).
struct WCombFillLaunch {
  uint32_t nkeys;
  uint64_t threads;
  size_t bases_off, comb_off;
};
template <int W>
inline WCombFillLaunch wcomb_fill_launch(uint32_t k0, uint32_t total, uint32_t batch) {
  using G = CombGeom<W>;
  const uint32_t nk = total - k0 < batch ? total - k0 : batch;
  return WCombFillLaunch{nk, (uint64_t)nk * G::kPos * G::kChunks, (size_t)k0 * G::kPos * 40,
                         (size_t)k0 * G::kWordsPerPoint};
}

#if defined(__HIPCC__)
// One thread per point (wcomb_key_bases); meta[key] gets the kKey* bits.
template <int W>
__global__ void k_wcomb_bases(const uint32_t* __restrict__ enc, uint32_t nkeys, int negate,
                              uint32_t* __restrict__ bases, uint32_t* __restrict__ meta, uint32_t* __restrict__ comb) {
  const uint32_t key = blockIdx.x * blockDim.x + threadIdx.x;
  if (key >= nkeys) return;
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = enc[8 * key + i];
  wcomb_key_bases<W>(w, negate, bases + (size_t)key * CombGeom<W>::kPos * 40,
                     comb + (size_t)key * CombGeom<W>::kWordsPerPoint + CombGeom<W>::kCorrWord, meta ? meta + key : nullptr);
}

// One thread per (key, position, chunk of 64 entries): wcomb_fill_target.
template <int W>
__global__ void k_wcomb_fill(const uint32_t* __restrict__ bases, uint32_t nkeys, uint32_t* __restrict__ comb,
                             uint32_t* __restrict__ tmp) {
  using G = CombGeom<W>;
  WCombFillTarget ft;
  if (!wcomb_fill_target<W>(ft, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nkeys)) return;
  wcomb_fill<W>(comb + ft.dst, tmp + ft.tmp, bases + ((size_t)ft.key * G::kPos + ft.pos) * 40, ft.chunk);
}

// Builds the W-bit wide combs of nkeys points, `batch` keys per fill launch (tmp
// must hold wcomb_fill_tmp_bytes_per_key(W) * batch bytes; bases nkeys *
// wcomb_bases_bytes_per_key(W)).
template <int W>
inline hipError_t wcomb_build(const uint32_t* d_enc, uint32_t nkeys, int negate, uint32_t* d_comb, uint32_t* d_meta,
                              uint32_t* d_bases, uint32_t* d_tmp, uint32_t batch, hipStream_t s) {
  hipLaunchKernelGGL(k_wcomb_bases<W>, dim3((nkeys + 63) / 64), dim3(64), 0, s, d_enc, nkeys, negate, d_bases,
                     d_meta, d_comb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  for (uint32_t k0 = 0; k0 < nkeys; k0 += batch) {
    const WCombFillLaunch fl = wcomb_fill_launch<W>(k0, nkeys, batch);
    hipLaunchKernelGGL(k_wcomb_fill<W>, dim3((uint32_t)((fl.threads + 63) / 64)), dim3(64), 0, s,
                       d_bases + fl.bases_off, fl.nkeys, d_comb + fl.comb_off, d_tmp);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
#endif  // __HIPCC__

}  // namespace nt
