// kernels_common.hpp -- definitions shared by the gfx950 kernel translation
// units (k_misc.hip, k_verify_*.hip, k_keyset_*.hip): block size, workspace
// layout, table accessors, and the occupancy-variant switch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "ed25519_ops.hpp"
#include "kernels.hpp"

namespace nt {

constexpr int kBlock = 256;

// Short kernels that run beside a long key-cache or verify launch of another
// stream (digests, key sort, verdict packing, group AND, wire parsing) raise
// their waves' issue priority on entry.  The SIMD arbiter otherwise prefers
// the older waves of the long launch, which is VALU-issue-bound: a 15 us
// certificate-digest launch on the next pipeline step then waits ~0.8 ms, for
// the other launch's tail (rocprofv3 trace).  -DNT_AUX_PRIO=0
// keeps the default priority (A/B).
#ifndef NT_AUX_PRIO
#define NT_AUX_PRIO 2
#endif
NT_D NT_INLINE void aux_priority() {
#if NT_AUX_PRIO
  __builtin_amdgcn_s_setprio(NT_AUX_PRIO);
#endif
}
#ifndef NT_VERIFY_PER_LANE
#define NT_VERIFY_PER_LANE 2
#endif
// signatures per lane per block iteration of k_ed25519_verify (1 or 2; A/B builds)
constexpr int kVPer = NT_VERIFY_PER_LANE;
constexpr int kAEntries = 18;         // j*(+-A) and j*(-R), |digit| in 0..8
constexpr int kAQuads = 10;           // uint4 per entry

// --------------------------------------------------------------------------
// Table accessors
// --------------------------------------------------------------------------
// N uint4 <-> 4 N words.  Quad i lies at p[i], or where the layout's own index expression
// at(i) says (KsStash: a fixed stride from quad 0 instead compiles to other addressing and
// another register allocation of the key-cache kernels).
template <int N, class At>
NT_D NT_INLINE void ld_quads_at(uint32_t* w, const At& at) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint4 v = *at(i);
    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
  }
}
template <int N, class At>
NT_D NT_INLINE void st_quads_at(const At& at, const uint32_t* w) {
#pragma unroll
  for (int i = 0; i < N; ++i) *at(i) = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
template <int N>
NT_D NT_INLINE void ld_quads(uint32_t* w, const uint4* p) {
  ld_quads_at<N>(w, [p](int i) { return p + i; });
}
template <int N>
NT_D NT_INLINE void st_quads(uint4* p, const uint32_t* w) {
  st_quads_at<N>([p](int i) { return p + i; }, w);
}
// 30 words <-> an affine niels entry, 40 words <-> a cached point
NT_D NT_INLINE void niels_of_words(ge_niels& q, const uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 10; ++i) { q.ypx.v[i] = w[i]; q.ymx.v[i] = w[10 + i]; q.xy2d.v[i] = w[20 + i]; }
}
NT_D NT_INLINE void words_of_niels(uint32_t* w, const ge_niels& q) {
#pragma unroll
  for (int i = 0; i < 10; ++i) { w[i] = q.ypx.v[i]; w[10 + i] = q.ymx.v[i]; w[20 + i] = q.xy2d.v[i]; }
}
NT_D NT_INLINE void cached_of_words(ge_cached& c, const uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 10; ++i) { c.YpX.v[i] = w[i]; c.YmX.v[i] = w[10 + i]; c.Z2.v[i] = w[20 + i]; c.T2d.v[i] = w[30 + i]; }
}
NT_D NT_INLINE void words_of_cached(uint32_t* w, const ge_cached& c) {
#pragma unroll
  for (int i = 0; i < 10; ++i) { w[i] = c.YpX.v[i]; w[10 + i] = c.YmX.v[i]; w[20 + i] = c.Z2.v[i]; w[30 + i] = c.T2d.v[i]; }
}

// Wide comb of one point with digit width W, layout [pos][entry][32 words];
// 8 x 16-byte loads.
template <int W>
struct WideComb {
  static constexpr int kBits = W;
  const uint32_t* base;
  NT_D NT_INLINE void load(uint32_t pos, uint32_t idx, ge_niels& q) const {
    uint32_t w[32];
    ld_quads<8>(w, (const uint4*)(base + ((size_t)pos * CombGeom<W>::kEntries + idx) * kWStride));
    niels_of_words(q, w);
  }
  // the point's [L]P entry after the positions (reduced-scalar combs, CombGeom::kCorrWord)
  NT_D NT_INLINE void load_corr(ge_niels& q) const {
    uint32_t w[32];
    ld_quads<8>(w, (const uint4*)(base + CombGeom<W>::kCorrWord));
    niels_of_words(q, w);
  }
};

// Per-lane point tables in the global workspace, uint4 granules, lane-major
// ([slot][lane][entry][quad]): an entry is 160 contiguous bytes of one lane, so
// the 10 loads of a table lookup use every byte of the ~1.5 lines they fetch.
// Why not lane-minor ([slot][entry][quad][lane]): a lookup's loads would
// coalesce only among lanes that picked the same entry -- with 9 entry
// magnitudes per 8-lane line that fetched ~5x the bytes used (PMC v7: 63 GB per
// 1M-verify launch, 5.5 TB/s).  Measured (same box, interleaved): lane-major
// 95.5 vs lane-minor 88.1 M verifies/s.
struct WsATab {
  uint4* ws;
  uint32_t slot;
  static constexpr uint32_t kEntries = kAEntries;  // what ktab_build_comb checks its 16 bases against
  NT_D NT_INLINE uint4* at(uint32_t entry) const {
    return ws + ((size_t)(slot * kBlock + threadIdx.x) * kAEntries + entry) * kAQuads;
  }
  NT_D NT_INLINE void load_signed(uint32_t e0, int32_t d, ge_cached& c) const {
    load(e0 + (uint32_t)(d < 0 ? -d : d), c);
    ge_cached_cneg(c, d < 0);
  }
  NT_D NT_INLINE void store(uint32_t entry, const ge_cached& c) const {
    uint32_t w[40];
    words_of_cached(w, c);
    st_quads<kAQuads>(at(entry), w);
  }
  NT_D NT_INLINE void load(uint32_t entry, ge_cached& c) const {
    uint32_t w[40];
    ld_quads<kAQuads>(w, at(entry));
    cached_of_words(c, w);
  }
};

// The x cache of the verify kernel (ed25519_ops.hpp XCache): `msk + 1` slots of
// two uint4 in global memory, one table per device entry, read and written by
// launches on any stream with no ordering between them -- a slot is only ever a
// candidate (ge_frombytes_x_check).  Callers keep every index <= msk, the
// allocated size - 1 (xcache_cand); tab == nullptr: no table (every wave takes
// the slow path, nothing is stored).
struct DevXCache {
  static constexpr bool kEnabled = true;
  uint4* tab;
  uint32_t msk;
  NT_D NT_INLINE bool active() const { return tab != nullptr; }
  NT_D NT_INLINE uint32_t mask() const { return msk; }
  NT_D NT_INLINE void load(uint32_t i, uint32_t xw[8]) const {
    const uint4* e = tab + 2 * (size_t)(i & msk);
    const uint4 a = e[0], b = e[1];
    xw[0] = a.x; xw[1] = a.y; xw[2] = a.z; xw[3] = a.w; xw[4] = b.x; xw[5] = b.y; xw[6] = b.z; xw[7] = b.w;
  }
  NT_D NT_INLINE void store(uint32_t i, const uint32_t xw[8]) const {
    uint4* e = tab + 2 * (size_t)(i & msk);
    e[0] = make_uint4(xw[0], xw[1], xw[2], xw[3]);
    e[1] = make_uint4(xw[4], xw[5], xw[6], xw[7]);
  }
};

// The key-table cache of the verify kernel (ktab.hpp) in global memory, one per
// device entry, read and written by launches on any stream with no ordering between them.
// Shared words (index slots, control block) are only ever touched by agent-scope atomics; pool
// entries by plain VECTOR accesses (per-lane addresses through a non-restrict pointer: never the
// scalar path) -- stored before the builder's drain + agent-scope release + slot store,
// loaded after the reader's slot loads + ONE agent-scope acquire.  Insert-only: a pool line is
// never read before a slot names its entry and never written after, and entries are 128-byte
// aligned multiples of 128 bytes, so no cache line a reader may hold goes stale.
// Indices: slots are masked here, entry indices are checked against cap by the callers
// (ktab_ready_index, ktab_build) before they get here, table and point numbers are clamped here.
// -DNT_KTAB4=0 (A/B builds): a three-table policy -- cached rows run verify_uv3 as before the
// fourth table, and nothing reads the extension pool.
// -DNT_KCOMB=0 (A/B builds): the second pool holds the fourth table and cached rows run verify_k4,
// kernel and allocation as before the comb; the default fills it with the keys' combs (verify_kc).
// NT_KTAB4=0 implies no comb.
#ifndef NT_KTAB4
#define NT_KTAB4 1
#endif
#ifndef NT_KCOMB
#define NT_KCOMB 1
#endif
struct DevKTab {
  static constexpr bool kEnabled = true;
  static constexpr uint32_t kEntryQuads = kKtEntryBytes / 16, kHeaderQuads = kKtHeaderBytes / 16;
  static_assert(kKtEntryBytes % 128 == 0 && kKtPointBytes == 160, "entry = whole 128-byte lines of 10-quad points");
  // One pointer and the launch's capacity are all a launch carries in registers.  base: the
  // control block (128 bytes: words 0..3 = entries handed out and the three row counters,
  // words 4..5 = the pool's address, word 6 = slots - 1, words 8..9 = the extension pool's
  // address; these five written once, before the first launch, and read here through the scalar
  // path: they are never handed off), then the index slots.
  uint32_t* base;
  uint32_t cap;
  NT_D NT_INLINE bool active() const { return base != nullptr; }
  NT_D NT_INLINE uint32_t slot_mask() const { return base[6]; }
  NT_D NT_INLINE uint32_t capacity() const { return cap; }
  NT_D NT_INLINE unsigned long long* slot_ptr(uint32_t i) const {
    return (unsigned long long*)(base + 32) + (i & slot_mask());
  }
  NT_D NT_INLINE uint4* pool_ptr() const { return (uint4*)(*(const unsigned long long*)(base + 4)); }
  NT_D NT_INLINE uint32_t* ctl_ptr() const { return base; }
  NT_D NT_INLINE uint64_t slot_load(uint32_t i) const {
    return __hip_atomic_load(slot_ptr(i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // returns the word found (== expect: the exchange happened)
  NT_D NT_INLINE uint64_t slot_cas(uint32_t i, uint64_t expect, uint64_t desired) const {
    unsigned long long e = expect;
    (void)__hip_atomic_compare_exchange_strong(slot_ptr(i), &e, (unsigned long long)desired, __ATOMIC_RELAXED,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return e;
  }
  // a lane's claimed slot while its balanced verification runs: LDS, not a register
  NT_D NT_INLINE uint32_t* claim_cell() const {
    __shared__ uint32_t s_claim[kBlock];
    return s_claim + threadIdx.x;
  }
  // the three-table ladder's 16 digit words, [word][thread]
  NT_D NT_INLINE uint32_t* dig_cell(uint32_t i) const {
    __shared__ uint32_t s_dig[16 * kBlock];
    return s_dig + (i & 15u) * kBlock + threadIdx.x;
  }
  NT_D NT_INLINE void dig_put(uint32_t i, uint32_t w) const { *dig_cell(i) = w; }
  NT_D NT_INLINE uint32_t dig_get(uint32_t i) const { return *dig_cell(i); }
  NT_D NT_INLINE void claim_put(uint32_t v) const { *claim_cell() = v; }
  NT_D NT_INLINE uint32_t claim_get() const { return *claim_cell(); }
  NT_D NT_INLINE void slot_store(uint32_t i, uint64_t w) const {
    __hip_atomic_store(slot_ptr(i), (unsigned long long)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // after drain_release(): the store that names a finished entry
  NT_D NT_INLINE void slot_publish(uint32_t i, uint64_t w) const { slot_store(i, w); }
  NT_D NT_INLINE void acquire() const { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
  // the storing wave: its vector stores drained, then the agent-scope release, then a drain of
  // the release's own write-back -- all before the slot store that follows
  NT_D NT_INLINE void drain_release() const {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  NT_D NT_INLINE uint32_t pool_used() const { return __hip_atomic_load(ctl_ptr(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  NT_D NT_INLINE uint32_t pool_take() const {
    return __hip_atomic_fetch_add(ctl_ptr(), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // once per wave row, by one lane
  NT_D NT_INLINE void count(int which) const {
    if ((threadIdx.x & 63u) == 0) __hip_atomic_fetch_add(ctl_ptr() + 1 + which, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  NT_D NT_INLINE uint4* entry(uint32_t idx) const { return pool_ptr() + (size_t)idx * kEntryQuads; }
  NT_D NT_INLINE uint4* point(uint32_t idx, uint32_t t, uint32_t j) const {
    return entry(idx) + kHeaderQuads + ((t % kKtTables) * kKtPerTable + ((j - 1u) & (kKtPerTable - 1u))) * 10u;
  }
  NT_D NT_INLINE void hdr_load(uint32_t idx, uint32_t tag[8], uint32_t& flags) const {
    const uint4* e = entry(idx);
    const uint4 a = e[0], b = e[1], c = e[2];
    tag[0] = a.x; tag[1] = a.y; tag[2] = a.z; tag[3] = a.w; tag[4] = b.x; tag[5] = b.y; tag[6] = b.z; tag[7] = b.w;
    flags = c.x;
  }
  NT_D NT_INLINE void hdr_store(uint32_t idx, const uint32_t tag[8], uint32_t flags) const {
    uint4* e = entry(idx);
    e[0] = make_uint4(tag[0], tag[1], tag[2], tag[3]);
    e[1] = make_uint4(tag[4], tag[5], tag[6], tag[7]);
    e[2] = make_uint4(flags, 0u, 0u, 0u);
  }
  // The extension pool: cap x kKtExtBytes, the fourth table ([2^192]A) of the entry with the
  // same index.  Its address is words 8..9 of the control block, written once beside words 4..6
  // and read the same way; zero = no fourth table (the callers ask has_ext() first: a null
  // extension is never dereferenced).
  // What the second pool holds is a compile-time choice: the key's comb (kComb, the default:
  // cap x kKtCombBytes, 33 lines of 128 B per entry index -- the window tables are then never
  // built for a key that gets an entry through verify_n, and has_ext() is false for good) or
  // the fourth table (-DNT_KCOMB=0).
  static constexpr bool kExt = NT_KTAB4 != 0;
  static constexpr bool kComb = NT_KTAB4 != 0 && NT_KCOMB != 0;
  static constexpr uint32_t kExtQuads = kKtExtBytes / 16, kCombQuads = kKtCombBytes / 16, kLineQuads = kKcLineBytes / 16;
  static_assert(kKtExtBytes % 128 == 0 && kKtCombBytes % 128 == 0, "second-pool entry = whole 128-byte lines");
  NT_D NT_INLINE uint4* ext_ptr() const { return (uint4*)(*(const unsigned long long*)(base + 8)); }
  NT_D NT_INLINE bool has_ext() const { return !kComb && ext_ptr() != nullptr; }
  NT_D NT_INLINE bool has_comb() const { return kComb && ext_ptr() != nullptr; }
  // comb line `entry` (clamped) of entry index idx: 7 quads and a half, bytes 120..127 are never written
  NT_D NT_INLINE uint4* comb_line(uint32_t idx, uint32_t entry) const {
    return ext_ptr() + (size_t)idx * kCombQuads + (entry < kKcEntries ? entry : kKcEntries - 1u) * kLineQuads;
  }
  NT_D NT_INLINE void comb_store(uint32_t idx, uint32_t entry, const ge_niels& q) const {
    uint32_t w[30];
    words_of_niels(w, q);
    uint4* p = comb_line(idx, entry);
    st_quads<7>(p, w);
    *(uint2*)(p + 7) = make_uint2(w[28], w[29]);
  }
  NT_D NT_INLINE void comb_load(uint32_t idx, uint32_t entry, ge_niels& q) const {
    uint32_t w[30];
    const uint4* p = comb_line(idx, entry);
    ld_quads<7>(w, p);
    const uint2 h = *(const uint2*)(p + 7);
    w[28] = h.x; w[29] = h.y;
    niels_of_words(q, w);
  }
  NT_D NT_INLINE uint4* ext_point(uint32_t idx, uint32_t j) const {
    return ext_ptr() + (size_t)idx * kExtQuads + ((j - 1u) & (kKtPerTable - 1u)) * 10u;
  }
  NT_D NT_INLINE void point_store(uint4* p, const ge_cached& c) const {
    uint32_t w[40];
    words_of_cached(w, c);
    st_quads<10>(p, w);
  }
  NT_D NT_INLINE void tab_store(uint32_t idx, uint32_t t, uint32_t j, const ge_cached& c) const {
    point_store(point(idx, t, j), c);
  }
  NT_D NT_INLINE void ext_store(uint32_t idx, uint32_t j, const ge_cached& c) const { point_store(ext_point(idx, j), c); }
  // point |d| of table t with the sign of d; d = 0: the identity, synthesized (the load still
  // goes to a valid point of the entry and is dropped)
  NT_D NT_INLINE void tab_load_signed(uint32_t idx, uint32_t t, int32_t d, ge_cached& c) const {
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    point_load_signed(point(idx, t, a), a, d < 0, c);
  }
  // the same of the fourth table
  NT_D NT_INLINE void ext_load_signed(uint32_t idx, int32_t d, ge_cached& c) const {
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    point_load_signed(ext_point(idx, a), a, d < 0, c);
  }
  NT_D NT_INLINE void point_load_signed(const uint4* p, uint32_t a, bool neg, ge_cached& c) const {
    uint32_t w[40];
    ld_quads<10>(w, p);
    ge_cached z;
    ge_cached_0(z);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      c.YpX.v[i] = a ? w[i] : z.YpX.v[i];
      c.YmX.v[i] = a ? w[10 + i] : z.YmX.v[i];
      c.Z2.v[i] = a ? w[20 + i] : z.Z2.v[i];
      c.T2d.v[i] = a ? w[30 + i] : z.T2d.v[i];
    }
    ge_cached_cneg(c, neg);
  }
};

// ---- key-cache verification: up to 64 signatures per lane, one inversion ----
#ifndef NT_KS_PER_LANE
#define NT_KS_PER_LANE 64
#endif
// most signatures per lane sharing one inversion; a launch runs
// keyset_per_lane() <= kKsPerLane of them (a kernel argument)
constexpr int kKsPerLane = NT_KS_PER_LANE;
constexpr int kKsQuads = 10;  // X, Y, Z, prefix: 40 words per (signature, lane)

// Per-lane stash in global memory, layout [wave][j][quad][lane] of uint4
// (lane-minor: a wave's 16-byte accesses are contiguous); a wave's region is
// (most rows of a chunk) * kKsQuads * 64 quads.
struct KsStash {
  uint4* base;  // this wave's region
  NT_D NT_INLINE uint4* at(int j, int q) const {
    return base + ((size_t)(j * kKsQuads + q) * 64 + (threadIdx.x & 63u));
  }
  NT_D NT_INLINE void put(int j, const ge_p2& P, const fe& a) const {
    uint32_t w[40];
#pragma unroll
    for (int i = 0; i < 10; ++i) { w[i] = P.X.v[i]; w[10 + i] = P.Y.v[i]; w[20 + i] = P.Z.v[i]; w[30 + i] = a.v[i]; }
    st_quads_at<kKsQuads>([&](int q) { return at(j, q); }, w);
  }
  NT_D NT_INLINE void get_point(int j, ge_p2& P) const {
    uint32_t w[32];
    ld_quads_at<8>(w, [&](int q) { return at(j, q); });
#pragma unroll
    for (int i = 0; i < 10; ++i) { P.X.v[i] = w[i]; P.Y.v[i] = w[10 + i]; P.Z.v[i] = w[20 + i]; }
  }
  NT_D NT_INLINE void get_prefix(int j, fe& a) const {
    uint32_t w[12];
    ld_quads_at<3>(w, [&](int q) { return at(j, 7 + q); });
#pragma unroll
    for (int i = 0; i < 10; ++i) a.v[i] = w[2 + i];
  }
};

// The launch's verdict epilogue (round 6): each signature's
// verdict goes straight into the caller's 64-bit words -- a ballot store when a
// row is one word (input order), an atomic OR of its bit when the launch runs
// in key-grouped order (no verdict bytes, no k_pack_bytes launch) -- and a
// rejected signature that lies in a certificate group clears that group's bit
// (the launch's init kernel set every group word to ones), so no k_group_and
// launch follows.  Groups: G ranges [gfirst[g], gfirst[g] + gcnt[g]) of the
// launch's signature indices (offset by ibase), gfirst non-decreasing; a
// signature in no group (a header signature of a mixed launch) only gets its bit.
struct KsVerdict {
  unsigned long long* bits;   // the launch's verdict words
  uint8_t* bytes;             // key-grouped order with the separate pack launch (NT_KEYSET_PACK=1), else null
  const uint64_t* gfirst;
  const uint32_t* gcnt;
  uint64_t G;
  unsigned long long* gwords;
  uint64_t ibase;             // index of the launch's signature 0 among the groups' indices

  NT_D NT_INLINE void group_fail(uint64_t i) const {
    const uint64_t x = ibase + i;
    if (G == 0 || gfirst[0] > x) return;
    uint64_t lo = 0, hi = G;  // the last group whose first index is <= x
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (gfirst[mid] <= x) lo = mid;
      else hi = mid;
    }
    if (x < gfirst[lo] + gcnt[lo]) atomicAnd(&gwords[lo >> 6], ~(1ull << (lo & 63)));
  }
  // signature i of the launch (key-grouped order: its own index), verdict ok
  NT_D NT_INLINE void scattered(uint64_t i, uint32_t ok) const {
    if (bytes) {
      bytes[i] = (uint8_t)ok;
    } else if (ok) {
      atomicOr(&bits[i >> 6], 1ull << (i & 63));
    }
    if (!ok) group_fail(i);
  }
  // row `row` of the launch in input order (lane = its signature), this lane's verdict ok
  NT_D NT_INLINE void row(uint64_t row, uint32_t lane, uint32_t ok, uint64_t n) const {
    const uint64_t gi = 64 * row + lane;
    const unsigned long long bal = __ballot(ok & (gi < n));
    if (lane == 0) bits[row] = bal;
    if (!ok && gi < n) group_fail(gi);
  }
};

// Per-mode launchers, explicitly instantiated in k_verify_<mode>.hip and
// k_keyset_<mode>.hip (one translation unit per kernel family and mode, so
// the build compiles them in parallel); dispatched by launch_verify /
// launch_verify_keyset in k_misc.hip.
// WB = digit width of the comb of B (kBCombBits or kBCombFallback), WA = the
// committee keys' comb width.
template <int MODE, int WB>
hipError_t launch_verify_m(uint64_t blocks, const uint8_t* d_pk, const uint8_t* d_sig, const uint8_t* d_msg,
                           uint64_t msg_bytes, const uint64_t* d_off, const uint64_t* d_len, uint64_t n,
                           const uint32_t* d_combB, void* d_ws, uint64_t* d_out_words, hipStream_t s, int per_lane,
                           XTab xt, KTabArgs kt);
template <int MODE, int WA, int WB>
hipError_t launch_keyset_m(const KsPlan& plan, const uint32_t* d_key_idx, const uint8_t* d_sig, const uint8_t* d_msg,
                           uint64_t msg_bytes, const uint64_t* d_off, const uint64_t* d_len, uint64_t n, const uint32_t* d_meta,
                           const uint32_t* d_enc, const uint32_t* d_combA, uint32_t nkeys,
                           const uint32_t* d_combB, void* d_stash, const uint32_t* d_perm, const KsVerdict& vd,
                           uint32_t* d_chunk_ctr, hipStream_t s);
int keyset_occupancy();

// Occupancy variants (waves per SIMD the register allocator targets), chosen
// at run time for A/B measurement: NT_VERIFY_OCC in {1, 2, 3} (default 2),
// NT_KEYSET_OCC in {2, 3} (default 3).
inline int env_occ(const char* name, int dflt, int lo, int hi) {
  const char* e = std::getenv(name);
  const int v = e ? std::atoi(e) : dflt;
  return v < lo || v > hi ? dflt : v;
}

}  // namespace nt
