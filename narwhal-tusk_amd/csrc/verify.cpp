// verify.cpp -- per-item verification: nt_ed25519_verify_strict (with and without the key
// registry) and nt_ed25519_verify_keyset.
#include "cpu_lane.hpp"
#include "pipeline.hpp"

namespace ntrt {
namespace {

// The shell of a per-item verify call on one shard: items [lo, lo + m) in the
// chunks `ch`, each chunk's messages, kw-byte keys and signatures copied on the
// copy stream (straight DMAs when all of them lie in nt_host_alloc memory),
// launch(c, a, b, ms) for chunk c = items [a, b), the verdict words of B_OUT
// copied back and packed into the caller's bitmap.
template <class Launch>
int verify_items(Device& dv, const Chunks& ch, uint64_t lo, size_t kw, const uint8_t* keys, const uint8_t* sig64,
                 const uint8_t* msg, const uint64_t* off, const uint64_t* len, uint8_t* out_bitmap, Launch&& launch) {
  const uint64_t m = ch.back().second, words = (m + 63) / 64;
  MsgStage ms;
  NT_CHK(msg_prepare(dv, off, len, lo, ch, ms));
  NT_CHK(dv.d[B_PK].ensure(m * kw));
  NT_CHK(dv.d[B_SIG].ensure(m * 64));
  NT_CHK(dv.d[B_OUT].ensure(words * 8));
  NT_CHK(dv.h[B_OUT].ensure(words * 8));
  const bool pinned = ms_pinned(ms, msg) && is_pinned(keys + kw * lo, kw * m) && is_pinned(sig64 + 64 * lo, 64 * m);
  NT_CHK(run_chunks(dv, ch.size(), pinned, [&](size_t c) -> int {
    const uint64_t a = ch[c].first, b = ch[c].second;
    NT_CHK(msg_copy(dv, msg, off, len, lo, ms, c, a, b));
    NT_TRY(hipMemcpyAsync(dv.d[B_PK].as<uint8_t>() + kw * a, keys + kw * (lo + a), (b - a) * kw,
                          hipMemcpyHostToDevice, dv.cstream));
    NT_TRY(hipMemcpyAsync(dv.d[B_SIG].as<uint8_t>() + 64 * a, sig64 + 64 * (lo + a), (b - a) * 64,
                          hipMemcpyHostToDevice, dv.cstream));
    return NT_OK;
  }, [&](size_t c) -> int { return launch(c, ch[c].first, ch[c].second, ms); }));
  NT_CHK(finish_chunks(dv));
  NT_TRY(hipMemcpyAsync(dv.h[B_OUT].p, dv.d[B_OUT].p, words * 8, hipMemcpyDeviceToHost, dv.lane[0].stream));
  NT_TRY(hipStreamSynchronize(dv.lane[0].stream));
  words_to_bitmap(out_bitmap + lo / 8, dv.h[B_OUT].as<uint64_t>(), m);
  return NT_OK;
}

}  // namespace

// nt_ed25519_verify_strict's GPU body: the uncached verify kernel over the
// shard's chunks (copies of chunk c + 1 under the kernels of chunk c)
int verify_strict_gpu(nt_ctx* ctx, const uint8_t* pk32, const uint8_t* sig64, const uint8_t* msg, const uint64_t* off,
                      const uint64_t* len, uint64_t n, uint8_t* out_bitmap) {
  return run_sharded(ctx, n, 64, [&](Device& dv, uint64_t lo, uint64_t hi) -> int {
    NT_CHK(verify_tables(dv));
    const uint64_t R1 = pipe_round(nt::verify_round_sigs(dv.cus, 1));
    const Chunks ch = nt::plan_chunks(verify_chunk_targets(hi - lo, R1));
    return verify_items(dv, ch, lo, 32, pk32, sig64, msg, off, len, out_bitmap,
                        [&](size_t c, uint64_t a, uint64_t b, const MsgStage& ms) -> int {
      // chunks of at most one round: one signature per lane (half the launch latency)
      return dv.verify_host(c, NT_MODE_STRICT, dv.d[B_PK].as<uint8_t>() + 32 * a,
                            dv.d[B_SIG].as<uint8_t>() + 64 * a, dv.d[B_DATA].as<uint8_t>(), ms.span,
                            chunk_off(dv, a), chunk_len(dv, a, b), b - a, dv.d[B_OUT].as<uint64_t>() + a / 64,
                            b - a <= R1 ? 1 : 0);
    });
  }, latency_sized(ctx, (n + ctx->devs.size() - 1) / ctx->devs.size(), nt::verify_round_sigs(ctx->devs[0]->cus)));
}

// key-cache verification of n (key index, signature, message) items against kd's tables
int verify_keyset_gpu(nt_ctx* ctx, const KeyDev& kd, int mode, const uint32_t* key_idx, const uint8_t* sig64,
                      const uint8_t* msg, const uint64_t* off, const uint64_t* len, uint64_t n, uint8_t* out_bitmap) {
  return run_sharded(ctx, n, 64, [&](Device& dv, uint64_t lo, uint64_t hi) -> int {
    NT_CHK(comb_b_for(dv));
    const nt::KsTabs tabs = ks_tabs(kd.t->dev[dv.group], kd.bits, kd.nkeys, dv);
    const Chunks ch = nt::plan_chunks(chunk_targets(hi - lo, pipe_round(nt::keyset_round_sigs(dv.cus))));
    // the scratch of every lane the chunks use, sized for the largest chunk before the pipeline starts
    uint64_t mc = 0;
    for (const auto& c : ch) mc = std::max(mc, c.second - c.first);
    for (size_t k = 0; k < std::min<size_t>(ch.size(), 2); ++k) NT_CHK(dv.ensure_scratch(dv.lane[k], mc));
    return verify_items(dv, ch, lo, 4, (const uint8_t*)key_idx, sig64, msg, off, len, out_bitmap,
                        [&](size_t c, uint64_t a, uint64_t b, const MsgStage& ms) -> int {
      Lane& l = dv.lane[c & 1];
      return dv.keyset_on(l, l.stream, mc, [&](nt::KsScratch scratch) {
        return nt::launch_verify_keyset(mode, tabs, scratch, dv.d[B_PK].as<uint32_t>() + a,
                                        dv.d[B_SIG].as<uint8_t>() + 64 * a, dv.d[B_DATA].as<uint8_t>(), ms.span,
                                        chunk_off(dv, a), chunk_len(dv, a, b), b - a,
                                        dv.d[B_OUT].as<uint64_t>() + a / 64, l.stream);
      });
    });
  }, latency_sized(ctx, (n + ctx->devs.size() - 1) / ctx->devs.size(), nt::keyset_round_sigs(ctx->devs[0]->cus)));
}

namespace {

// Registry lookups (key_table.hpp) of n consecutive 32-byte keys into kid (nt::kKeyMiss where
// the index does not hold the key), split by pool_split; returns the misses
uint64_t reg_lookup(const nt::KeyTable& tab, const uint8_t* pk, uint64_t n, uint32_t* kid) {
  uint64_t m = 0;
  for (uint64_t x : pool_split<uint64_t>(n, [&](uint64_t lo, uint64_t hi) {
         uint64_t miss = 0;
         for (uint64_t i = lo; i < hi; ++i) {
           kid[i] = tab.find(pk + 32 * i);
           miss += kid[i] == nt::kKeyMiss;
         }
         return miss;
       }))
    m += x;
  return m;
}

// up to kRegNoteMax keys of the items that missed (kid null: of every item), for the registry's sightings
std::vector<const uint8_t*> missed_keys(const uint8_t* pk, uint64_t n, const uint32_t* kid) {
  std::vector<const uint8_t*> v;
  for (uint64_t i = 0; i < n && v.size() < 4 * kRegNoteMax; ++i)
    if (!kid || kid[i] == nt::kKeyMiss) v.push_back(pk + 32 * i);
  return v;
}

// a small call on the host lane: item(i) = the verdict of item i, packed into out_bitmap
template <class F>
int host_items(nt_ctx* ctx, uint64_t n, uint8_t* out_bitmap, F&& item) {
  std::vector<uint8_t> ok(n);
  nt::cpu::parallel_for(n, small_threads(ctx, n), [&](uint64_t i) { ok[i] = item(i); });
  std::memset(out_bitmap, 0, (n + 7) / 8);
  for (uint64_t i = 0; i < n; ++i)
    if (ok[i]) nt::byte_put(out_bitmap, i, true);
  ctx->calls_host++;
  return NT_OK;
}

// verify_strict with the registry's snapshot: every item through the key-cache
// kernel in strict mode (a missed key carries kKeyMiss: unknown, reject), then
// the misses through the uncached kernel, their verdicts merged
int verify_strict_reg(nt_ctx* ctx, const RegSnap& snap, const std::vector<uint32_t>& kid, uint64_t miss,
                      const uint8_t* pk32, const uint8_t* sig64, const uint8_t* msg, const uint64_t* off,
                      const uint64_t* len, uint64_t n, uint8_t* out_bitmap) {
  NT_CHK0(verify_keyset_gpu(ctx, snap.dev(), NT_MODE_STRICT, kid.data(), sig64, msg, off, len, n, out_bitmap));
  if (!miss) return NT_OK;
  std::vector<uint64_t> idx;
  idx.reserve(miss);
  uint64_t bytes = 0, mn = UINT64_MAX, mx = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (kid[i] == nt::kKeyMiss) {
      idx.push_back(i);
      bytes += len[i];
      if (len[i]) {
        mn = std::min(mn, off[i]);
        mx = std::max(mx, off[i] + len[i]);
      }
    }
  const uint64_t M = idx.size();
  std::vector<uint8_t> pk(32 * M), sg(64 * M), bm((M + 7) / 8 + 1);
  std::vector<uint64_t> o(M), l(M);
  // the misses' messages: gathered when they are a small part of the span they
  // lie in (a few scattered misses must not copy the whole buffer), else in place
  const bool gather = mn < mx && bytes < (mx - mn) / 4;
  std::vector<uint8_t> gm(gather ? bytes + 1 : 0);
  uint64_t at = 0;
  for (uint64_t j = 0; j < M; ++j) {
    const uint64_t i = idx[j];
    std::memcpy(pk.data() + 32 * j, pk32 + 32 * i, 32);
    std::memcpy(sg.data() + 64 * j, sig64 + 64 * i, 64);
    l[j] = len[i];
    if (gather) {
      if (len[i]) std::memcpy(gm.data() + at, msg + off[i], len[i]);
      o[j] = at;
      at += len[i];
    } else {
      o[j] = off[i];
    }
  }
  NT_CHK0(verify_strict_gpu(ctx, pk.data(), sg.data(), gather ? gm.data() : msg, o.data(), l.data(), M, bm.data()));
  for (uint64_t j = 0; j < M; ++j) nt::byte_put(out_bitmap, idx[j], nt::byte_bit(bm.data(), j));
  return NT_OK;
}

}  // namespace
}  // namespace ntrt

using namespace ntrt;

extern "C" {

int nt_ed25519_verify_strict(nt_ctx* ctx, const uint8_t* pk32, const uint8_t* sig64,
                             const uint8_t* msg, const uint64_t* off, const uint64_t* len,
                             uint64_t n, uint8_t* out_bitmap) {
  if (!ctx || (n && (!pk32 || !sig64 || !off || !len || !out_bitmap))) return NT_EINVAL;
  if (n == 0) return NT_OK;
  // the key registry (nt_set_key_cache): registered keys through the key cache
  std::shared_ptr<const RegSnap> snap = ctx->reg ? reg_snapshot(ctx) : nullptr;
  std::vector<uint32_t> kid;
  uint64_t miss = n;
  if (snap) {
    kid.resize(n);
    miss = reg_lookup(snap->table, pk32, n, kid.data());
    reg_count(ctx, n - miss, miss);
  }
  if (ctx->reg && miss) reg_note_misses(ctx, missed_keys(pk32, n, snap ? kid.data() : nullptr));
  const bool cached = snap && miss < n;
  if (small_verify(ctx, n, cached && !miss ? nt::kRouteKeyCache : nt::kRouteUncached))
    return host_items(ctx, n, out_bitmap, [&](uint64_t i) {
      return nt::cpu::verify(nt::kStrict, pk32 + 32 * i, sig64 + 64 * i, msg + off[i], len[i]);
    });
  ctx->calls_gpu++;
  if (cached) return verify_strict_reg(ctx, *snap, kid, miss, pk32, sig64, msg, off, len, n, out_bitmap);
  return verify_strict_gpu(ctx, pk32, sig64, msg, off, len, n, out_bitmap);
}

int nt_ed25519_verify_keyset(nt_ctx* ctx, const nt_keyset* ks, int mode, const uint32_t* key_idx,
                             const uint8_t* sig64, const uint8_t* msg, const uint64_t* off,
                             const uint64_t* len, uint64_t n, uint8_t* out_bitmap) {
  if (!ctx || !ks || ks->ctx != ctx || (mode != NT_MODE_STRICT && mode != NT_MODE_COFACTORLESS && mode != NT_MODE_MIXED))
    return NT_EINVAL;
  if (n && (!key_idx || !sig64 || !off || !len || !out_bitmap)) return NT_EINVAL;
  if (n == 0) return NT_OK;
  if (small_verify(ctx, n, nt::kRouteKeyCache))
    return host_items(ctx, n, out_bitmap, [&](uint64_t i) {
      uint8_t A[32];
      const int m = keyset_key(ks, mode, key_idx[i], A);
      return m >= 0 && nt::cpu::verify(m, A, sig64 + 64 * i, msg + off[i], len[i]);
    });
  ctx->calls_gpu++;
  return verify_keyset_gpu(ctx, KeyDev{ks->t.get(), ks->bits, ks->nkeys}, mode, key_idx, sig64, msg, off, len, n,
                           out_bitmap);
}

}  // extern "C"
