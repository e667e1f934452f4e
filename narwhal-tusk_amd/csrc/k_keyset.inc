// k_keyset.inc -- verification against a committee key cache and its per-mode
// launcher; included by k_keyset_strict.hip and k_keyset_cofactorless.hip.
// The key-cache kernels are compiled without the scheduling fence after each
// field multiply that the verify kernel keeps (fe25519.hpp): interleaved A/B
// on the final round-3 build (profiles/r03/ab_fence/), config 3 +0.6 % in 3 of
// 3 rounds, config 2 unchanged with the fence removed (-0.2 %).
// -DNT_KEYSET_MUL_FENCE restores it.
#if !defined(NT_KEYSET_MUL_FENCE) && !defined(NT_NO_MUL_FENCE)
#define NT_NO_MUL_FENCE 1
#endif
#include "kernels_common.hpp"

namespace nt {

// Inputs of signature j of this lane: wave w, lane l handles signatures
// 64 m w + 64 j + l, j < m = per_lane (so each verdict word is one ballot);
// key_idx[i] selects the key (>= nkeys -> unknown key -> reject).
template <int MODE, int WA>
struct KsLoader {
  using Comb = WideComb<WA>;
  const uint32_t* key_idx;
  const uint32_t* sig;
  const uint8_t* msg;
  uint64_t msg_bytes;
  const uint64_t* off;
  const uint64_t* len;
  uint64_t n, base;
  const uint32_t* perm;  // key-grouped order (launch_verify_keyset): slot -> signature, or null
  const uint32_t* meta;
  const uint32_t* enc;
  const uint32_t* combA;
  uint32_t nkeys, lane;
  NT_D NT_INLINE uint64_t index(int j) const {
    const uint64_t gi = base + 64 * (uint64_t)j + lane;
    const uint64_t s = gi < n ? gi : n - 1;
    return perm ? perm[s] : s;
  }
  NT_D NT_INLINE void get(int j, uint32_t& m, uint32_t Aw[8], uint32_t Rw[8], uint32_t Sw[8], const uint8_t*& mp,
                          uint64_t& ln, Comb& ca) const {
    const uint64_t i = index(j);
    uint32_t kraw = key_idx[i];
    uint32_t want_strict = 0;
    if (MODE == kMixed) {  // bit 31 = this signature is checked strictly
      want_strict = kraw & kKeyWantStrict;
      kraw &= ~kKeyWantStrict;
    }
    const MsgSlice ms = msg_slice(off[i], len[i], msg_bytes);
    const uint32_t known = kraw < nkeys;
    const uint32_t key = known ? kraw : 0u;
    // an unknown key or an out-of-bounds message: no key flags, so the signature rejects
    m = (known & ms.ok ? meta[key] : 0u) | want_strict;
    ld8(Aw, enc + 8 * key);
    ld8(Rw, sig + 16 * i);
    ld8(Sw, sig + 16 * i + 8);
    mp = msg + ms.off;
    ln = ms.len;
    ca = Comb{combA + key * CombGeom<WA>::kWordsPerPoint};
  }
  NT_D NT_INLINE void rbytes(int j, uint32_t Rw[8]) const { ld8(Rw, sig + 16 * index(j)); }
};

// Verification against a cached committee, persistent and balanced.  The
// launch's R = ceil(n / 64) rows of 64 signatures (one per lane) are cut into
// `chunks` consecutive chunks, the first `extra` of them base + 1 rows, the
// rest base rows (launch_verify_keyset: chunks = k x waves, at most kKsPerLane
// rows each, so every wave runs k equal-sized chunks and no SIMD is left with
// a lone tail wave).  A wave claims chunk indices from a counter until they
// run out: the loop ends for every wave once the counter passes `chunks`.
// Within a chunk each lane verifies its rows' signatures with ONE inversion
// (verify_cached_batch), R'_j and the prefix products staged in this wave's
// stash region.
template <int MODE, int OCC, int WA, int WB>
__global__ __launch_bounds__(kBlock, OCC) void k_ed25519_verify_keyset(
    const uint32_t* __restrict__ key_idx, const uint32_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint64_t msg_bytes, const uint64_t* __restrict__ off, const uint64_t* __restrict__ len, uint64_t n,
    const uint32_t* __restrict__ meta, const uint32_t* __restrict__ enc, const uint32_t* __restrict__ combA,
    uint32_t nkeys, const uint32_t* __restrict__ combB, uint4* __restrict__ stash, const uint32_t* __restrict__ perm,
    const KsVerdict vd, uint32_t* __restrict__ chunk_ctr, uint32_t waves, uint32_t chunks, uint32_t base_rows,
    uint32_t extra) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  if (wave >= waves) return;  // the last block's surplus waves (no stash region)
  const uint32_t pmax = base_rows + (extra ? 1u : 0u);
  const KsStash st{stash + (size_t)wave * pmax * kKsQuads * 64};
#pragma unroll 1
  for (;;) {
    uint32_t c = 0;
    if (lane == 0) c = atomicAdd(chunk_ctr, 1u);  // one claim per wave (a vector atomic)
    c = __shfl(c, 0);
    if (c >= chunks) break;
    const int m = (int)(base_rows + (c < extra ? 1u : 0u));
    const uint64_t row0 = (uint64_t)c * base_rows + (c < extra ? c : extra);
    const uint64_t base = 64 * row0;
    const KsLoader<MODE, WA> ld{key_idx, sig, msg, msg_bytes, off, len, n, base, perm, meta, enc, combA, nkeys, lane};
    const uint64_t bits = verify_cached_batch<MODE, kKsPerLane>(ld, WideComb<WB>{combB}, st, m);
#pragma unroll 1
    for (int j = 0; j < m; ++j) {
      const uint64_t gi = base + 64 * j + lane;
      const uint32_t ok = (uint32_t)(bits >> j) & 1u;
      if (perm) {  // key-grouped order: the verdict at the signature's own index
        if (gi < n) vd.scattered(perm[gi], ok);
      } else if (base + 64 * j < n) {
        vd.row((base >> 6) + j, lane, ok, n);
      }
    }
  }
}

// Streamed rows (ks_stream_plan): a wave claims one row at a time -- the claim
// of the next row is issued before the current row runs, so its latency is
// hidden -- and stages up to `prow` rows' R' and Z prefix products in its
// stash; when the counter passes `rows` (or the stash is full) it inverts once
// and finishes its rows backwards, reading their row indices from LDS.  Same
// per-signature arithmetic as verify_cached_batch (ed25519_ops.hpp).
template <int MODE, int OCC, int WA, int WB>
__global__ __launch_bounds__(kBlock, OCC) void k_ed25519_verify_keyset_stream(
    const uint32_t* __restrict__ key_idx, const uint32_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint64_t msg_bytes, const uint64_t* __restrict__ off, const uint64_t* __restrict__ len, uint64_t n,
    const uint32_t* __restrict__ meta, const uint32_t* __restrict__ enc, const uint32_t* __restrict__ combA,
    uint32_t nkeys, const uint32_t* __restrict__ combB, uint4* __restrict__ stash, const uint32_t* __restrict__ perm,
    const KsVerdict vd, uint32_t* __restrict__ row_ctr, uint32_t waves, uint32_t rows, uint32_t prow) {
  // a wave batches at most prow <= kKsPerLane rows (launch_keyset_m checks it): one
  // LDS slot per row for its index, one bit per row in the 64-bit verdict masks
  static_assert(kKsPerLane >= 1 && kKsPerLane <= 64, "verdict masks of a wave batch are 64-bit words");
  __shared__ uint32_t s_rows[kBlock / 64][kKsPerLane];
  const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
  const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  if (wave >= waves) return;  // the last block's surplus waves (no stash region)
  const KsStash st{stash + (size_t)wave * prow * kKsQuads * 64};
  uint32_t claim = 0;
  if (lane == 0) claim = atomicAdd(row_ctr, 1u);
  uint32_t r = __builtin_amdgcn_readfirstlane(claim);
#pragma unroll 1
  for (;;) {
    uint64_t okbits = 0, strictbits = 0;
    fe acc;
    fe_1(acc);
    int m = 0;
#pragma unroll 1
    while (r < rows && m < (int)prow) {
      if (lane == 0) claim = atomicAdd(row_ctr, 1u);  // the next row; read after this one
      s_rows[wib][m] = r;
      const KsLoader<MODE, WA> ld{key_idx, sig, msg, msg_bytes, off, len, n, 64 * (uint64_t)r, perm, meta, enc, combA, nkeys, lane};
      uint32_t mt, Aw[8], Rw[8], Sw[8];
      const uint8_t* mp;
      uint64_t ln;
      typename KsLoader<MODE, WA>::Comb ca;
      ld.get(0, mt, Aw, Rw, Sw, mp, ln, ca);
      ge_p3 P;
      okbits |= (uint64_t)cached_point<MODE>(P, mt, Aw, Rw, Sw, mp, ln, ca, WideComb<WB>{combB}) << m;
      strictbits |= (uint64_t)(is_strict<MODE>(mt) ? 1u : 0u) << m;
      if (m == 0) acc = P.Z;
      else fe_mul(acc, acc, P.Z);
      ge_p2 P2;
      ge_p3_to_p2(P2, P);
      st.put(m, P2, acc);
      ++m;
      r = __builtin_amdgcn_readfirstlane(claim);
    }
    const bool last = r >= rows;  // wave-uniform: the counter ran out (else the stash is full)
    fe inv;
    if (m == 0) break;
    fe_invert_batch(inv, acc);
#pragma unroll 1
    for (int j = m - 1; j >= 0; --j) {
      ge_p2 P;
      fe zi;
      st.get_point(j, P);
      if (j > 0) {
        fe pre;
        st.get_prefix(j - 1, pre);  // Z_0 .. Z_{j-1}
        fe_mul(zi, inv, pre);
        fe_mul(inv, inv, P.Z);
      } else {
        zi = inv;
      }
      const uint64_t row = s_rows[wib][j];
      const KsLoader<MODE, WA> ld{key_idx, sig, msg, msg_bytes, off, len, n, 64 * row, perm, meta, enc, combA, nkeys, lane};
      uint32_t Rw[8];
      ld.rbytes(0, Rw);
      const uint32_t ok = (uint32_t)(okbits >> j) & compare_one<MODE>(P, zi, Rw, (strictbits >> j) & 1u);
      const uint64_t gi = 64 * row + lane;
      if (perm) {  // key-grouped order: the verdict at the signature's own index
        if (gi < n) vd.scattered(perm[gi], ok);
      } else {
        vd.row(row, lane, ok, n);
      }
    }
    if (last) break;
  }
}

template <int MODE, int WA, int WB>
hipError_t launch_keyset_m(const KsPlan& pl, const uint32_t* d_key_idx, const uint8_t* d_sig, const uint8_t* d_msg,
                           uint64_t msg_bytes, const uint64_t* d_off, const uint64_t* d_len, uint64_t n, const uint32_t* d_meta,
                           const uint32_t* d_enc, const uint32_t* d_combA, uint32_t nkeys,
                           const uint32_t* d_combB, void* d_stash, const uint32_t* d_perm, const KsVerdict& vd,
                           uint32_t* d_ctr, hipStream_t s) {
  const uint32_t blocks = (pl.waves + kBlock / 64 - 1) / (kBlock / 64);
#define NT_KS_LAUNCH(O)                                                                                     \
  hipLaunchKernelGGL((k_ed25519_verify_keyset<MODE, O, WA, WB>), dim3(blocks), dim3(kBlock), 0, s, d_key_idx,      \
                     (const uint32_t*)d_sig, d_msg, msg_bytes, d_off, d_len, n, d_meta, d_enc, d_combA, nkeys, d_combB,    \
                     (uint4*)d_stash, d_perm, vd, d_ctr, pl.waves, pl.chunks, pl.base_rows, pl.extra)
#define NT_KS_LAUNCH_STREAM(O)                                                                              \
  hipLaunchKernelGGL((k_ed25519_verify_keyset_stream<MODE, O, WA, WB>), dim3(blocks), dim3(kBlock), 0, s, d_key_idx, \
                     (const uint32_t*)d_sig, d_msg, msg_bytes, d_off, d_len, n, d_meta, d_enc, d_combA, nkeys, d_combB,    \
                     (uint4*)d_stash, d_perm, vd, d_ctr, pl.waves, pl.rows, pl.prow)
  // the register budget of the variant caps the resident waves per SIMD at the plan's count
  if (pl.stream) {
    if (pl.prow < 1 || pl.prow > (uint32_t)kKsPerLane) return hipErrorInvalidValue;
    // NT_KEYSET_LEAN=1 (A/B): the 3-waves-per-SIMD build (84 VGPRs) also for
    // plans of 1-2 waves per SIMD, leaving more of a SIMD's registers to a
    // co-resident launch of another stream
    static const bool lean = [] {
      const char* e = std::getenv("NT_KEYSET_LEAN");
      return e && *e == '1';
    }();
    if (pl.per_simd >= 3 || lean) NT_KS_LAUNCH_STREAM(3);
    else NT_KS_LAUNCH_STREAM(2);
  } else if (pl.per_simd >= 3) {
    NT_KS_LAUNCH(3);
  } else {
    NT_KS_LAUNCH(2);
  }
#undef NT_KS_LAUNCH
#undef NT_KS_LAUNCH_STREAM
  return hipGetLastError();
}

}  // namespace nt
