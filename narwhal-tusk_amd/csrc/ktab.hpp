// ktab.hpp -- the key-table cache (KTab) of the verify kernel: what is kept for
// a public key seen before, the index protocol (probe / mark / claim / take)
// and the policy contract.  A part of ed25519_ops.hpp, which includes it after
// the x cache and verify_uv: include that file, not this one.  What a cached
// row runs over an entry is in ktab_comb.hpp (the comb: what the product runs)
// and ktab_tables.hpp (the window tables of the earlier generations).
#pragma once

namespace nt {

// ---------------------------------------------------------------------------
// The key-table cache (KTab): for a public key this context has seen before, precomputed
// multiples of A kept across calls, so that a row whose keys are all cached needs far fewer
// doublings than the balanced path (verify_uv).  What an entry holds is the policy's choice:
//   the key's comb in the second pool (kComb, the default: verify_kc, ktab_comb.hpp) -- only
//   the entry's header is then written to the first pool, no window table is built;
//   four window tables, the fourth in the second pool (kExt without kComb: verify_k4), or
//   three window tables and the unbalanced lattice vector (neither: verify_uv3), both in
//   ktab_tables.hpp.
// Every one of them sums an integer identity over real multiples of A, so the verdict is
// verify_uv's for every input.
//
// Storage (the verify kernel: DevKTab, kernels_common.hpp; the host harness: plain
// memory and host atomics):
//   pool   entries of kKtEntryBytes: a 128-B header (the 32 key bytes as tag,
//          kKt* flags) + 3 tables x 8 cached points of 160 B.  Insert-only: an
//          entry is handed out once by a bump counter and never rewritten or
//          freed while the context lives.
//   index  8-byte slots {fingerprint32, state32}; a key has two buckets of
//          kKtBucket slots (half a 128-B line each) from two hashes.
//   state  0 empty -> kKtSeen (first sighting: one CAS, nothing else)
//          -> kKtClaimed (second sighting: CAS, one winner per key, who builds
//          the entry after its verification) -> kKtReady0 + entry index.
//          Pool exhausted: the slot stays kKtSeen.
// Soundness.  A pool line is never read before the slot that names it has been
// read as ready, the builder stores the whole entry, drains, releases at agent
// scope and only then stores the slot word, and the reader acquires at agent
// scope between the slot loads and the first pool load: together with
// insert-only this means a reader sees either no entry or the finished one.  A
// stale slot read is only a miss.  The header's full 32-byte tag is compared
// before a table is used, so a fingerprint collision is a miss as well, and
// every index is masked (slots) or bounds-checked (entries) before use.
// A wave row takes the fast path only when all its lanes hit.
//
// Policy (KT):
//   kEnabled, active(), slot_mask() (slots - 1, a power of two >= kKtBucket),
//   capacity() (entries), slot_load / slot_cas / slot_store / slot_publish,
//   acquire(), drain_release(), pool_used(), pool_take(), hdr_load / hdr_store,
//   tab_store(idx, t, j, c), tab_load_signed(idx, t, d, c), count(which),
//   claim_put / claim_get (what a lane owes the cache after its row, parked outside
//   its registers while the balanced path runs), dig_put / dig_get (the 16 digit
//   words of the three-table ladder, likewise; the comb's ladder parks its 9 there)
// and, for the policies that say so, the fourth table's or the comb's accessors (below).
// ---------------------------------------------------------------------------
constexpr uint32_t kKtTables = 3, kKtPerTable = 8;
constexpr uint32_t kKtHeaderBytes = 128, kKtPointBytes = 160;
constexpr uint32_t kKtEntryBytes = kKtHeaderBytes + kKtTables * kKtPerTable * kKtPointBytes;  // 3,968
constexpr uint32_t kKtBucket = 8;             // slots per bucket (64 bytes)
constexpr uint32_t kKtCand = 2 * kKtBucket;   // slots a probe reads
constexpr uint32_t kKtSeen = 1, kKtClaimed = 2, kKtReady0 = 16;  // slot states; ready: kKtReady0 + index
constexpr uint32_t kKtNoSlot = 0xffffffffu;
constexpr uint32_t kKtWantMark = 0xfffffffeu;  // parked beside a claimed slot: mark this key after the row
constexpr uint32_t kKtWantTake = 0xfffffffdu;  // ... or claim it outright: the x cache has met it before
constexpr uint32_t kKtFlagShift = 28, kKtMaxEntries = 1u << kKtFlagShift;  // entry index | flags in one word
enum : uint32_t { kKtUndecodable = 1u, kKtSmallOrder = 2u };  // header flags
enum { kKtCntFast = 0, kKtCntBuild = 1, kKtCntOld = 2 };      // counters: wave rows

// The fourth table, A''' = [2^192]A, lives outside the entry, in an extension pool
// of kKtExtBytes per entry index (8 cached points: ten 128-B lines).  With it the
// whole 253-bit k splits into four strings of 16 digits and the cached verify needs
// no lattice vector and nothing of R but its bytes (verify_k4).  A policy says that
// it can carry one with `static constexpr bool kExt = true` and then has
//   has_ext() (wave-uniform: an extension pool is there), ext_store(idx, j, c),
//   ext_load_signed(idx, d, c)
// Policies without the member are three-table policies: nothing below asks them for more.
constexpr uint32_t kKtExtBytes = kKtPerTable * kKtPointBytes;  // 1,280
template <class KT>
constexpr auto kt_ext_of(int) -> decltype(KT::kExt) { return KT::kExt; }
template <class KT>
constexpr bool kt_ext_of(long) { return false; }
template <class KT>
constexpr bool kKtHasExt = kt_ext_of<KT>(0);
// an extension pool is there (wave-uniform)
template <class KT>
NT_HD NT_INLINE bool ktab_has_ext(const KT& kt) {
  if constexpr (kKtHasExt<KT>) return kt.has_ext();
  else return false;
}

// The second pool may instead hold the key's comb: a policy says so with `static constexpr
// bool kComb = true` (ktab_comb.hpp, "The comb": the layout and what such a policy provides).
template <class KT>
constexpr auto kt_comb_of(int) -> decltype(KT::kComb) { return KT::kComb; }
template <class KT>
constexpr bool kt_comb_of(long) { return false; }
template <class KT>
constexpr bool kKtHasComb = kt_comb_of<KT>(0);
// the second pool is there and holds combs (wave-uniform)
template <class KT>
NT_HD NT_INLINE bool ktab_has_comb(const KT& kt) {
  if constexpr (kKtHasComb<KT>) return kt.has_comb();
  else return false;
}

// What a row whose lanes all hit runs, by what the policy carries and which pools are there
// (wave-uniform, and the same for every launch of a context): the comb's ladder (verify_kc), the
// four-table ladder (verify_k4), the three-table ladder over the unbalanced vector (verify_uv3),
// or nothing -- a policy that can carry a fourth table has none of them without its second pool.
// The gate and the dispatch of verify_one_kt both ask here.
enum : uint32_t { kKtFastNone = 0, kKtFastThree = 3, kKtFastFour = 4, kKtFastComb = 5 };
template <class KT>
NT_HD NT_INLINE uint32_t ktab_fast_kind(const KT& kt) {
  if constexpr (kKtHasComb<KT>) {
    if (kt.has_comb()) return kKtFastComb;
  }
  if constexpr (kKtHasExt<KT>) return kt.has_ext() ? kKtFastFour : kKtFastNone;
  else return kKtFastThree;
}

struct NoKTab {
  static constexpr bool kEnabled = false;
  NT_HD NT_INLINE bool active() const { return false; }
  NT_HD NT_INLINE uint32_t slot_mask() const { return 0; }
  NT_HD NT_INLINE uint32_t capacity() const { return 0; }
  NT_HD NT_INLINE uint64_t slot_load(uint32_t) const { return 0; }
  NT_HD NT_INLINE uint64_t slot_cas(uint32_t, uint64_t, uint64_t) const { return ~0ull; }  // returns the old word
  NT_HD NT_INLINE void dig_put(uint32_t, uint32_t) const {}
  NT_HD NT_INLINE uint32_t dig_get(uint32_t) const { return 0; }
  NT_HD NT_INLINE void claim_put(uint32_t) const {}
  NT_HD NT_INLINE uint32_t claim_get() const { return 0xffffffffu; }
  NT_HD NT_INLINE void slot_store(uint32_t, uint64_t) const {}
  NT_HD NT_INLINE void slot_publish(uint32_t, uint64_t) const {}
  NT_HD NT_INLINE void acquire() const {}
  NT_HD NT_INLINE void drain_release() const {}
  NT_HD NT_INLINE uint32_t pool_used() const { return 0; }
  NT_HD NT_INLINE uint32_t pool_take() const { return 0; }
  NT_HD NT_INLINE void hdr_load(uint32_t, uint32_t*, uint32_t&) const {}
  NT_HD NT_INLINE void hdr_store(uint32_t, const uint32_t*, uint32_t) const {}
  NT_HD NT_INLINE void tab_store(uint32_t, uint32_t, uint32_t, const ge_cached&) const {}
  NT_HD NT_INLINE void tab_load_signed(uint32_t, uint32_t, int32_t, ge_cached&) const {}
  NT_HD NT_INLINE void count(int) const {}
};

// a key's fingerprint in its index slot
NT_HD NT_INLINE uint32_t ktab_fp(const uint32_t Aw[8]) { return xcache_hash(Aw, 0x94d049bbu); }
NT_HD NT_INLINE uint64_t ktab_word(uint32_t fp, uint32_t st) { return (uint64_t)fp | ((uint64_t)st << 32); }

// What a probe found: the key's fingerprint, the state and slot of its match
// (st = 0: none) and the empty slots a first sighting may take: bit c of `ord` =
// slot c of the emptier bucket (base pb), bit 8 + c = slot c of the other (base
// ob); ord = 0: both buckets full -- the key stays homeless.
struct KtProbe {
  uint32_t fp, st, slot, pb, ob, ord;
};

// 16 relaxed slot loads (two buckets of 8: two rounds of loads in flight together)
template <class KT>
NT_HD NT_INLINE void ktab_probe(KtProbe& p, const uint32_t Aw[8], const KT& kt) {
  const uint32_t mask = kt.slot_mask(), bm = mask / kKtBucket;
  const uint32_t b0 = (xcache_hash(Aw, 0x51ed270bu) & bm) * kKtBucket;
  const uint32_t b1 = (xcache_hash(Aw, 0x2545f491u) & bm) * kKtBucket;
  p.fp = ktab_fp(Aw);
  p.st = 0;
  p.slot = 0;
  uint64_t w[kKtCand];
#pragma unroll
  for (uint32_t c = 0; c < kKtCand; ++c) w[c] = kt.slot_load(((c < kKtBucket ? b0 : b1) | (c & (kKtBucket - 1))) & mask);
  uint32_t emp = 0;
#pragma unroll
  for (uint32_t c = 0; c < kKtCand; ++c) {
    const uint32_t hi = (uint32_t)(w[c] >> 32);
    emp |= (w[c] == 0 ? 1u : 0u) << c;
    if (hi != 0 && (uint32_t)w[c] == p.fp && hi > p.st) {  // the furthest state wins (a key marked twice)
      p.st = hi;
      p.slot = ((c < kKtBucket ? b0 : b1) | (c & (kKtBucket - 1))) & mask;
    }
  }
  // two-choice placement: the emptier bucket first
  const uint32_t e0 = emp & ((1u << kKtBucket) - 1u), e1 = emp >> kKtBucket;
  const bool second = __builtin_popcount(e1) > __builtin_popcount(e0);
  p.pb = second ? b1 : b0;
  p.ob = second ? b0 : b1;
  p.ord = second ? (e1 | (e0 << kKtBucket)) : (e0 | (e1 << kKtBucket));
}

// The entry index of a ready match below the launch's capacity; kKtNoSlot otherwise.
template <class KT>
NT_HD NT_INLINE uint32_t ktab_ready_index(const KtProbe& p, const KT& kt) {
  const uint32_t idx = p.st - kKtReady0;
  return (p.st >= kKtReady0 && idx < kt.capacity()) ? idx : kKtNoSlot;
}

// The mark of a key that has no slot (p.st == 0): kKtSeen by CAS into the first slot the
// probe saw empty.  A mark that loses its CAS to another key (a batch of new keys fills its
// buckets at once) takes the next slot the probe saw empty, three tries in all and nothing
// re-read; one that loses to a lane with the same key is done.
// A mark is a partial write to a line no cache holds, acknowledged from the memory side, and
// the wave waits for it with its next loads: a launch whose every lane marks at once queues
// ~1.5 ns per mark behind one another (measured: 200 k marks, +0.3 ms).
// So a key the x cache meets for the first time writes nothing here -- that sighting is
// recorded for nothing by the x cache, which stores the key's x then -- and a key the x cache
// has met before is claimed outright and built (ktab_take); only keys of which the x cache can
// say nothing go through the mark (ge_frombytes_cached's `seen`).  Keys that never come back
// never pay.
template <class KT>
NT_HD NT_INLINE void ktab_mark(const KtProbe& p, const KT& kt) {
  uint32_t ord = p.ord;
#pragma unroll 1
  for (int a = 0; a < 3 && ord != 0; ++a) {
    const uint32_t c = (uint32_t)__builtin_ctz(ord);
    ord &= ord - 1u;
    const uint32_t i = ((c < kKtBucket ? p.pb : p.ob) | (c & (kKtBucket - 1))) & kt.slot_mask();
    const uint64_t old = kt.slot_cas(i, 0, ktab_word(p.fp, kKtSeen));
    if (old == 0 || (uint32_t)old == p.fp) break;
  }
}
// The claim of a key marked before: returns 1 for the one winner of the CAS, who builds the
// entry after its verification (ktab_build).  A claimed or ready slot and a full pool are left
// as they are.
template <class KT>
NT_HD NT_INLINE uint32_t ktab_claim(const KtProbe& p, const KT& kt) {
  if (p.st == kKtSeen && kt.pool_used() < kt.capacity())
    return kt.slot_cas(p.slot, ktab_word(p.fp, kKtSeen), ktab_word(p.fp, kKtClaimed)) == ktab_word(p.fp, kKtSeen) ? 1u : 0u;
  return 0;
}
// A slot for a key that has none, claimed outright (the x cache vouches for an earlier
// meeting): returns the slot won, kKtNoSlot otherwise.
template <class KT>
NT_HD NT_INLINE uint32_t ktab_take(const KtProbe& p, const KT& kt) {
  if (p.st != 0) return ktab_claim(p, kt) ? p.slot : kKtNoSlot;
  if (kt.pool_used() >= kt.capacity()) return kKtNoSlot;
  uint32_t ord = p.ord;
#pragma unroll 1
  for (int a = 0; a < 3 && ord != 0; ++a) {
    const uint32_t c = (uint32_t)__builtin_ctz(ord);
    ord &= ord - 1u;
    const uint32_t i = ((c < kKtBucket ? p.pb : p.ob) | (c & (kKtBucket - 1))) & kt.slot_mask();
    const uint64_t old = kt.slot_cas(i, 0, ktab_word(p.fp, kKtClaimed));
    if (old == 0) return i;
    if ((uint32_t)old == p.fp) break;
  }
  return kKtNoSlot;
}
// Mark or claim in one, for a caller that has no x cache to ask.
template <class KT>
NT_HD NT_INLINE uint32_t ktab_sight(const KtProbe& p, const KT& kt) {
  if (p.st == 0) {
    ktab_mark(p, kt);
    return 0;
  }
  return ktab_claim(p, kt);
}
// ge_frombytes_cached's `seen` for a lane parked as kKtWantMark: a key the x cache meets for
// the first time is not marked this time
template <class KT>
struct KtSeenSink {
  const KT& kt;
  NT_HD NT_INLINE void operator()(uint32_t known) const {
    if (KT::kEnabled && known != 1u && kt.claim_get() == kKtWantMark) kt.claim_put(known ? kKtWantTake : kKtNoSlot);
  }
};

}  // namespace nt
