// groups.cpp -- certificate groups: nt_ed25519_verify_batch_groups and its key-set form.
#include "cpu_lane.hpp"
#include "group_plan.hpp"
#include "pipeline.hpp"

using namespace ntrt;

namespace {

// certificate groups on host threads: per-signature rule, AND per group.
// key(e, A) writes signature e's key encoding to A and returns its mode
// (kStrict / kCofactorless) or -1 for "no such key" (reject).
template <class KeyOf>
int host_groups(nt_ctx* ctx, const uint8_t* sig64, const uint64_t* first, const uint32_t* cnt, const uint8_t* msg32,
                uint64_t G, uint8_t* out_group_bitmap, uint8_t* out_sig_bitmap, KeyOf&& key) {
  std::vector<uint64_t> gbase(G + 1, 0);
  uint64_t nsig_total = 0;
  for (uint64_t g = 0; g < G; ++g) {
    gbase[g + 1] = gbase[g] + cnt[g];
    nsig_total = std::max(nsig_total, first[g] + cnt[g]);
  }
  const uint64_t m = gbase[G];
  std::vector<uint8_t> ok(m, 0);
  nt::cpu::parallel_for(m, small_threads(ctx, m), [&](uint64_t e) {
    const uint64_t g = (uint64_t)(std::upper_bound(gbase.begin(), gbase.end(), e) - gbase.begin()) - 1;
    const uint64_t s = first[g] + (e - gbase[g]);
    uint8_t A[32];
    const int mode = key(s, A);
    ok[e] = mode >= 0 && nt::cpu::verify(mode, A, sig64 + 64 * s, msg32 + 32 * g, 32);
  });
  std::memset(out_group_bitmap, 0, (G + 7) / 8);
  if (out_sig_bitmap) std::memset(out_sig_bitmap, 0, (nsig_total + 7) / 8);
  for (uint64_t g = 0; g < G; ++g) {
    bool all = true;
    for (uint64_t e = gbase[g]; e < gbase[g + 1]; ++e) {
      all = all && ok[e];
      if (out_sig_bitmap && ok[e]) nt::byte_put(out_sig_bitmap, first[g] + (e - gbase[g]), true);
    }
    if (all) nt::byte_put(out_group_bitmap, g, true);
  }
  ctx->calls_host++;
  return NT_OK;
}

// Gather the keys (kw bytes each; null hkey: none) and signatures of groups
// [g0, g1) back to back into pinned staging; start = the groups' first
// signatures within the chunk.  Copies are split over host threads by signature
// count (a config-3 batch stages ~0.6 GB; one thread would take ~50 ms of it).
void gather_groups(uint64_t g0, uint64_t g1, const uint64_t* first, const uint32_t* cnt, const uint64_t* start,
                   uint64_t m, size_t kw, const uint8_t* keys, const uint8_t* sig64, uint8_t* hkey, uint8_t* hsig) {
  const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const unsigned T = m < (1u << 16) ? 1u : hw;
  auto work = [&](unsigned t) {
    // groups whose first compacted signature falls in this thread's share
    const uint64_t slo = m * t / T, shi = m * (t + 1) / T;
    uint64_t j = (uint64_t)(std::lower_bound(start, start + (g1 - g0), slo) - start);
    for (; j < g1 - g0 && start[j] < shi; ++j) {
      const uint64_t g = g0 + j, c = cnt[g];
      if (!c) continue;
      if (hkey) std::memcpy(hkey + kw * start[j], keys + kw * first[g], kw * c);
      std::memcpy(hsig + 64 * start[j], sig64 + 64 * first[g], 64 * c);
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < T; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
}

// keys one call reports to the registry as sightings, at most
constexpr size_t kSightingsMax = 4 * kRegNoteMax;

// One groups call, shared by its shards: the caller's arrays in one of three key forms
//   kd == nullptr        32-byte encodings, the uncached verify kernel (cofactorless);
//   kd, tab == nullptr   4-byte committee indices into kd's tables (the key-cache kernel);
//   kd and tab           32-byte encodings looked up in the registry index `tab` on
//                        host threads as each chunk is staged, so the chunk carries 4-byte
//                        indices (68 B per vote over PCIe instead of 96); the signatures
//                        whose key misses verify afterwards through the uncached kernel
//                        and their groups' verdicts are recomputed (`missed`: their keys).
struct GroupCall {
  const KeyDev* kd;
  const nt::KeyTable* tab;
  const uint8_t* keys;
  const uint8_t* sig64;
  const uint64_t* first;
  const uint32_t* cnt;
  const uint8_t* msg32;
  uint8_t* out_group_bitmap;
  uint8_t* out_sig_bitmap;
  std::vector<const uint8_t*> missed;  // keys of signatures that missed (registry sightings)
  std::atomic<uint64_t> nmiss{0};
  std::mutex mu;  // out_sig_bitmap (shards share its bytes) and missed

  size_t kw() const { return kd && !tab ? 4 : 32; }  // key bytes per signature in the caller's array
  size_t kdv() const { return kd ? 4 : 32; }         // ... and on the device
};

// One shard of a groups call on one execution slot.  Groups are staged chunk by
// chunk into pinned memory (host threads) and copied on the copy stream; chunk
// c's verify and group-AND launches wait only for chunk c's copies.
class GroupShardRun {
 public:
  GroupShardRun(GroupCall& call, Device& dev) : a(call), dv(dev) {}

  int run(uint64_t glo, uint64_t ghi) {
    NT_CHK(a.kd ? comb_b_for(dv) : verify_tables(dv));
    NT_CHK(reserve(glo, ghi));
    NT_TRY(hipMemsetAsync(dv.d[B_OUT].p, 0, p.sw * 8 + 8, dv.cstream));  // before chunk 0's copy-done event
    if (a.tab && p.m) {
      stage_meta(0, p.chunks());  // the lookups read the group starts
      ahead.start(p.chunks(), [this](size_t c) {
        if (p.sigs(c)) lookup(c);
      });
    }
    // direct from pinned memory: every copy is a DMA, so chunk c+1's copies are
    // queued before the host waits on chunk c; direct from pageable memory: chunk
    // c's kernels are launched before chunk c+1's (synchronous) copies; gathered
    // or looked up: a helper thread stages (host memcpy of keys and signatures,
    // waits for the chunk's registry lookups) and issues the chunks ahead of the
    // launches (run_chunks_staged)
    auto cp = [this](size_t c) { return copy(c); };
    auto ln = [this](size_t c) { return launch(c); };
    NT_CHK(!a.tab && (direct || p.m == 0) ? run_chunks(dv, p.chunks(), direct_pinned || p.m == 0, cp, ln)
                                          : run_chunks_staged(dv, p.chunks(), cp, ln));
    NT_CHK(read_back());
    if (!miss.empty()) NT_CHK(resolve_misses());
    write_out();
    return NT_OK;
  }

 private:
  GroupCall& a;
  Device& dv;
  nt::GroupShard p;
  // densely packed keys and signatures are copied straight from the caller's
  // arrays: a DMA from nt_host_alloc memory, or HIP's own staged copy from
  // pageable memory (which returns when it is done: run_chunks' staged order);
  // scattered groups are gathered into the pinned staging on a helper thread.
  // Registry lookups always write their indices into the pinned staging, on the
  // look-ahead thread ahead of the copies.
  bool direct = false, direct_pinned = false;
  // header digests from pageable memory go through the pinned staging too (32 B
  // per group): a copy from pageable memory returns only when it is done
  bool msg_direct = false;
  nt::KsTabs tabs{};  // of a.kd on this slot
  uint8_t *hkey = nullptr, *hsig = nullptr, *hmsg = nullptr;
  const uint64_t* hfirst = nullptr;  // = p.start, in pinned memory
  uint32_t* hcnt = nullptr;
  std::vector<std::vector<nt::GroupMiss>> miss_c;  // per chunk; written by the look-ahead thread only
  std::vector<nt::GroupMiss> miss;                 // all of them, once the chunks are done
  // Registry lookups run on a thread of their own, chunk by chunk ahead of the
  // copies: a pageable signature copy (HIP stages it and returns when it is
  // done) of chunk c then overlaps the lookups of chunk c + 1.  (The last
  // member: its thread, which writes miss_c, is joined before anything else goes.)
  LookAhead ahead;

  // the plan and every buffer of the shard's first pass
  int reserve(uint64_t glo, uint64_t ghi) {
    const uint64_t gm = ghi - glo;
    uint64_t m = 0;
    for (uint64_t g = glo; g < ghi; ++g) m += a.cnt[g];
    const uint64_t R = pipe_round(a.kd ? nt::keyset_round_sigs(dv.cus) : nt::verify_round_sigs(dv.cus));
    NT_CHK(dv.h[B_FIRST].ensure(gm * 8));
    NT_CHK(dv.h[B_CNT].ensure(gm * 4));
    p = nt::plan_group_shard(glo, ghi, a.first, a.cnt, chunk_targets(m, R), dv.h[B_FIRST].as<uint64_t>());
    hfirst = p.start;
    hcnt = dv.h[B_CNT].as<uint32_t>();
    const size_t kw = a.kw(), kdv = a.kdv();
    const uint64_t mm = std::max<uint64_t>(m, 1);
    direct = p.direct;
    direct_pinned = direct && (a.tab || is_pinned(a.keys + kw * a.first[glo], kw * m)) &&
                    is_pinned(a.sig64 + 64 * a.first[glo], 64 * m);
    if (direct && !direct_pinned && std::getenv("NT_GROUPS_GATHER")) direct = false;  // A/B: round-5 staging
    msg_direct = is_pinned(a.msg32 + 32 * glo, 32 * gm);
    NT_CHK(dv.h[B_PK].ensure(a.tab ? mm * 4 : (direct ? 1 : mm * kw)));
    NT_CHK(dv.h[B_SIG].ensure(direct ? 1 : mm * 64));
    NT_CHK(dv.h[B_DATA].ensure(msg_direct ? 1 : gm * 32));
    NT_CHK(dv.h[B_OUT].ensure(p.sw * 8 + 8));
    NT_CHK(dv.h[B_OUT2].ensure(p.gw * 8));
    NT_CHK(dv.d[B_PK].ensure(mm * kdv));
    NT_CHK(dv.d[B_SIG].ensure(mm * 64));
    NT_CHK(dv.d[B_OFF].ensure(mm * 8));
    NT_CHK(dv.d[B_LEN].ensure(mm * 8));
    NT_CHK(dv.d[B_DATA].ensure(gm * 32 + 64));
    NT_CHK(dv.d[B_FIRST].ensure(gm * 8));
    NT_CHK(dv.d[B_CNT].ensure(gm * 4));
    NT_CHK(dv.d[B_OUT].ensure(p.sw * 8 + 8));
    NT_CHK(dv.d[B_OUT2].ensure(p.gw * 8));
    if (a.kd) {
      for (size_t k = 0; k < std::min<size_t>(p.chunks(), 2); ++k) NT_CHK(dv.ensure_scratch(dv.lane[k], p.max_chunk));
      tabs = ks_tabs(a.kd->t->dev[dv.group], a.kd->bits, a.kd->nkeys, dv);
    }
    hkey = dv.h[B_PK].as<uint8_t>();
    hsig = dv.h[B_SIG].as<uint8_t>();
    hmsg = dv.h[B_DATA].as<uint8_t>();
    miss_c.resize(p.chunks());
    return NT_OK;
  }

  // chunk-local group starts and counts of chunks [c0, c1) into the pinned staging
  void stage_meta(size_t c0, size_t c1) {
    for (size_t c = c0; c < c1; ++c) p.fill_starts(c, a.cnt);
    const uint64_t g0 = p.ch[c0].first, g1 = p.ch[c1 - 1].second;
    std::memcpy(hcnt + (g0 - p.glo), a.cnt + g0, (g1 - g0) * 4);
  }

  // registry lookups of chunk c's keys into hkey (4-byte indices; kKeyMiss = unknown)
  void lookup(size_t c) {
    const uint64_t g0 = p.ch[c].first, ng = p.ch[c].second - g0;
    const uint64_t* hf = hfirst + (g0 - p.glo);  // chunk-local group starts
    uint32_t* kid = (uint32_t*)hkey + p.E[c];
    for (auto& v : pool_split<std::vector<nt::GroupMiss>>(p.sigs(c), [&](uint64_t lo, uint64_t hi) {
           std::vector<nt::GroupMiss> part;
           uint64_t j = (uint64_t)(std::upper_bound(hf, hf + ng, lo) - hf) - 1;
           for (uint64_t e = lo; e < hi; ++e) {
             while (e >= hf[j] + a.cnt[g0 + j]) ++j;
             const uint32_t q = (uint32_t)(e - hf[j]);
             kid[e] = a.tab->find(a.keys + 32 * (a.first[g0 + j] + q));
             if (kid[e] == nt::kKeyMiss) part.push_back(nt::GroupMiss{g0 + j, (uint32_t)c, q});
           }
           return part;
         }))
      miss_c[c].insert(miss_c[c].end(), v.begin(), v.end());
  }

  // chunk c's inputs on the copy stream (device offsets chunk-local: the group
  // starts relative to E[c], message offsets 32 * (g - g0) made on the device)
  int copy(size_t c) {
    const uint64_t g0 = p.ch[c].first, ng = p.ch[c].second - g0, gl = g0 - p.glo, e0 = p.E[c], mc = p.sigs(c);
    const size_t kw = a.kw(), kdv = a.kdv();
    hipStream_t cs = dv.cstream;
    if (!a.tab || p.m == 0) stage_meta(c, c + 1);
    if (!direct && mc)
      gather_groups(g0, g0 + ng, a.first, a.cnt, hfirst + gl, mc, kw, a.keys, a.sig64,
                    a.tab ? nullptr : hkey + kw * e0, hsig + 64 * e0);
    // the signatures first: they do not depend on the registry lookups, so their
    // copy (94 % of a registry chunk's bytes) runs while the chunk's lookups finish
    if (mc) {
      const uint8_t* ss = direct ? a.sig64 + 64 * (a.first[p.glo] + e0) : hsig + 64 * e0;
      NT_TRY(hipMemcpyAsync(dv.d[B_SIG].as<uint8_t>() + 64 * e0, ss, mc * 64, hipMemcpyHostToDevice, cs));
    }
    if (a.tab && mc) ahead.wait(c);
    if (mc) {
      const uint8_t* sk = a.tab ? hkey + 4 * e0 : direct ? a.keys + kw * (a.first[p.glo] + e0) : hkey + kw * e0;
      NT_TRY(hipMemcpyAsync(dv.d[B_PK].as<uint8_t>() + kdv * e0, sk, mc * kdv, hipMemcpyHostToDevice, cs));
    }
    const uint8_t* sm = a.msg32 + 32 * g0;
    if (!msg_direct) {
      std::memcpy(hmsg + 32 * gl, sm, ng * 32);
      sm = hmsg + 32 * gl;
    }
    NT_TRY(hipMemcpyAsync(dv.d[B_DATA].as<uint8_t>() + 32 * gl, sm, ng * 32, hipMemcpyHostToDevice, cs));
    NT_TRY(hipMemcpyAsync(dv.d[B_FIRST].as<uint64_t>() + gl, hfirst + gl, ng * 8, hipMemcpyHostToDevice, cs));
    NT_TRY(hipMemcpyAsync(dv.d[B_CNT].as<uint32_t>() + gl, hcnt + gl, ng * 4, hipMemcpyHostToDevice, cs));
    return NT_OK;
  }

  // chunk c's kernels on its compute stream: message offsets, verify, the AND per group
  int launch(size_t c) {
    const uint64_t g0 = p.ch[c].first, ng = p.ch[c].second - g0, gl = g0 - p.glo, e0 = p.E[c], mc = p.sigs(c);
    hipStream_t s = dv.cstr((int)c);
    const uint8_t* dk = dv.d[B_PK].as<uint8_t>() + a.kdv() * e0;
    const uint8_t* dsig = dv.d[B_SIG].as<uint8_t>() + 64 * e0;
    const uint8_t* dmsg = dv.d[B_DATA].as<uint8_t>() + 32 * gl;
    uint64_t* doff = dv.d[B_OFF].as<uint64_t>() + e0;
    uint64_t* dlen = dv.d[B_LEN].as<uint64_t>() + e0;
    const uint64_t* dfirst = dv.d[B_FIRST].as<uint64_t>() + gl;
    const uint32_t* dcnt = dv.d[B_CNT].as<uint32_t>() + gl;
    uint64_t* dout = dv.d[B_OUT].as<uint64_t>() + p.W[c];
    uint64_t* dgout = dv.d[B_OUT2].as<uint64_t>() + gl / 64;
    if (mc) {
      NT_TRY(nt::launch_group_msgs(dfirst, dcnt, ng, doff, dlen, s));
      if (a.kd) {
        // the key-cache launch ANDs the chunk's groups itself (its kernel's epilogue)
        return dv.keyset_on(dv.lane[c & 1], s, p.max_chunk, [&](nt::KsScratch scratch) {
          return nt::launch_verify_keyset(NT_MODE_COFACTORLESS, tabs, scratch, (const uint32_t*)dk, dsig, dmsg, 32 * ng,
                                          doff, dlen, mc, dout, s, nt::KsGroups{dfirst, dcnt, ng, dgout});
        });
      }
      NT_CHK(dv.verify_host(c, NT_MODE_COFACTORLESS, dk, dsig, dmsg, 32 * ng, doff, dlen, mc, dout));
    }
    NT_TRY(nt::launch_group_and(dfirst, dcnt, ng, dout, dgout, s));
    return NT_OK;
  }

  uint64_t* sbits() const { return dv.h[B_OUT].as<uint64_t>(); }
  uint64_t* gbits() const { return dv.h[B_OUT2].as<uint64_t>(); }

  // every chunk done: the misses collected, the verdict words on the host
  int read_back() {
    NT_CHK(finish_chunks(dv));
    ahead.join();  // every chunk's lookups are done: miss_c is final
    for (auto& v : miss_c) miss.insert(miss.end(), v.begin(), v.end());
    NT_TRY(hipMemcpyAsync(gbits(), dv.d[B_OUT2].p, p.gw * 8, hipMemcpyDeviceToHost, dv.lane[0].stream));
    if ((a.out_sig_bitmap || !miss.empty()) && p.m)
      NT_TRY(hipMemcpyAsync(sbits(), dv.d[B_OUT].p, p.sw * 8, hipMemcpyDeviceToHost, dv.lane[0].stream));
    NT_TRY(hipStreamSynchronize(dv.lane[0].stream));
    return NT_OK;
  }

  // the keys the registry does not hold: the uncached kernel over just those
  // signatures (each over its group's digest, already on the device), then
  // their bits set and their groups' verdicts recomputed on the host
  int resolve_misses() {
    const uint64_t M = miss.size();
    hipStream_t s = dv.lane[0].stream;
    a.nmiss += M;
    NT_CHK(verify_tables(dv));
    NT_CHK(dv.h[B_PK].ensure(M * 32));
    NT_CHK(dv.h[B_SIG].ensure(M * 64));
    NT_CHK(dv.h[B_OFF].ensure(M * 16));
    NT_CHK(dv.d[B_PK].ensure(M * 32));
    NT_CHK(dv.d[B_SIG].ensure(M * 64));
    NT_CHK(dv.d[B_OFF].ensure(M * 16));
    NT_CHK(dv.d[B_OUT2].ensure(((M + 63) / 64) * 8));
    uint8_t* pk = dv.h[B_PK].as<uint8_t>();
    uint8_t* sg = dv.h[B_SIG].as<uint8_t>();
    uint64_t* ol = dv.h[B_OFF].as<uint64_t>();
    for (uint64_t j = 0; j < M; ++j) {
      const uint64_t o = a.first[miss[j].g] + miss[j].t;
      std::memcpy(pk + 32 * j, a.keys + 32 * o, 32);
      std::memcpy(sg + 64 * j, a.sig64 + 64 * o, 64);
      ol[j] = 32 * (miss[j].g - p.glo);
      ol[M + j] = 32;
    }
    NT_TRY(hipMemcpyAsync(dv.d[B_PK].p, pk, M * 32, hipMemcpyHostToDevice, s));
    NT_TRY(hipMemcpyAsync(dv.d[B_SIG].p, sg, M * 64, hipMemcpyHostToDevice, s));
    NT_TRY(hipMemcpyAsync(dv.d[B_OFF].p, ol, M * 16, hipMemcpyHostToDevice, s));
    const uint64_t R1 = nt::verify_round_sigs(dv.cus, 1);
    NT_CHK(dv.verify_host(0, NT_MODE_COFACTORLESS, dv.d[B_PK].as<uint8_t>(), dv.d[B_SIG].as<uint8_t>(),
                          dv.d[B_DATA].as<uint8_t>(), 32 * p.groups(), dv.d[B_OFF].as<uint64_t>(),
                          dv.d[B_OFF].as<uint64_t>() + M, M, dv.d[B_OUT2].as<uint64_t>(), M <= R1 ? 1 : 0));
    std::vector<uint64_t> mw((M + 63) / 64);
    NT_TRY(hipMemcpyAsync(mw.data(), dv.d[B_OUT2].p, mw.size() * 8, hipMemcpyDeviceToHost, s));
    NT_TRY(hipStreamSynchronize(s));
    nt::merge_group_misses(p, a.cnt, miss, mw.data(), sbits(), gbits());
    std::lock_guard<std::mutex> lk(a.mu);
    for (uint64_t j = 0; j < M && a.missed.size() < kSightingsMax; ++j)
      a.missed.push_back(a.keys + 32 * (a.first[miss[j].g] + miss[j].t));
    return NT_OK;
  }

  // the shard's verdicts into the caller's bitmaps
  void write_out() {
    words_to_bitmap(a.out_group_bitmap + p.glo / 8, gbits(), p.groups());
    if (!a.out_sig_bitmap || !p.m) return;
    std::lock_guard<std::mutex> lk(a.mu);
    nt::scatter_sig_bits(p, a.first, a.cnt, sbits(), a.out_sig_bitmap);
  }
};

// certificate groups [0, G) of `a` on the GPU, sharded over the context's device entries
int verify_groups(nt_ctx* ctx, GroupCall& a, uint64_t G) {
  uint64_t nsig_total = 0;
  for (uint64_t g = 0; g < G; ++g) nsig_total = std::max(nsig_total, a.first[g] + a.cnt[g]);
  if (nsig_total && (!a.keys || !a.sig64)) return NT_EINVAL;
  if (a.out_sig_bitmap) std::memset(a.out_sig_bitmap, 0, (nsig_total + 7) / 8);
  const uint64_t round = a.kd ? nt::keyset_round_sigs(ctx->devs[0]->cus) : nt::verify_round_sigs(ctx->devs[0]->cus);
  return run_sharded(ctx, G, 64, [&](Device& dv, uint64_t glo, uint64_t ghi) -> int {
    return GroupShardRun(a, dv).run(glo, ghi);
  }, latency_sized(ctx, (nsig_total + ctx->devs.size() - 1) / ctx->devs.size(), round));
}

// Up to kSightingsMax keys of the groups' signatures for the registry's
// sightings: those the index `tab` does not hold (tab null: every key)
std::vector<const uint8_t*> group_sightings(const nt::KeyTable* tab, const uint8_t* pk32, const uint64_t* first,
                                            const uint32_t* cnt, uint64_t G) {
  std::vector<const uint8_t*> ks;
  for (uint64_t g = 0; g < G; ++g)
    for (uint32_t q = 0; q < cnt[g]; ++q) {
      if (ks.size() >= kSightingsMax) return ks;
      const uint8_t* p = pk32 + 32 * (first[g] + q);
      if (!tab || tab->find(p) == nt::kKeyMiss) ks.push_back(p);
    }
  return ks;
}

// any key of the groups' signatures the registry index does not hold
bool groups_miss(const nt::KeyTable& tab, const uint8_t* pk32, const uint64_t* first, const uint32_t* cnt,
                 uint64_t G) {
  for (uint64_t g = 0; g < G; ++g)
    for (uint32_t q = 0; q < cnt[g]; ++q)
      if (tab.find(pk32 + 32 * (first[g] + q)) == nt::kKeyMiss) return true;
  return false;
}

}  // namespace

extern "C" {

int nt_ed25519_verify_batch_groups(nt_ctx* ctx, const uint8_t* pk32, const uint8_t* sig64,
                                   const uint64_t* first, const uint32_t* cnt,
                                   const uint8_t* msg32, uint64_t G, uint8_t* out_group_bitmap,
                                   uint8_t* out_sig_bitmap) {
  if (!ctx || (G && (!first || !cnt || !msg32 || !out_group_bitmap))) return NT_EINVAL;
  if (G == 0) return NT_OK;
  uint64_t m = 0, nsig = 0;
  for (uint64_t g = 0; g < G; ++g) {
    m += cnt[g];
    nsig = std::max(nsig, first[g] + cnt[g]);
  }
  if (m && (!pk32 || !sig64)) return NT_EINVAL;
  // the key registry (nt_set_key_cache): route by the kernel the call would run --
  // the key cache when every key hits, the uncached kernel otherwise
  std::shared_ptr<const RegSnap> snap = ctx->reg ? reg_snapshot(ctx) : nullptr;
  bool host = small_verify(ctx, m, snap ? nt::kRouteKeyCache : nt::kRouteUncached);
  if (!host && snap && small_verify(ctx, m, nt::kRouteUncached)) host = groups_miss(snap->table, pk32, first, cnt, G);
  if (host) {
    // sightings of the keys the registry does not hold yet
    if (ctx->reg) reg_note_misses(ctx, group_sightings(snap ? &snap->table : nullptr, pk32, first, cnt, G));
    return host_groups(ctx, sig64, first, cnt, msg32, G, out_group_bitmap, out_sig_bitmap,
                       [&](uint64_t s, uint8_t A[32]) {
                         std::memcpy(A, pk32 + 32 * s, 32);
                         return (int)nt::kCofactorless;
                       });
  }
  ctx->calls_gpu++;
  if (snap) {
    const KeyDev kd = snap->dev();
    GroupCall a{&kd, &snap->table, pk32, sig64, first, cnt, msg32, out_group_bitmap, out_sig_bitmap};
    const int rc = verify_groups(ctx, a, G);
    const uint64_t nmiss = a.nmiss.load();
    reg_count(ctx, m - std::min(m, nmiss), nmiss);
    if (!a.missed.empty()) reg_note_misses(ctx, a.missed);
    return rc;
  }
  // an empty registry: the first keys of the call are its first sightings
  if (ctx->reg) reg_note_misses(ctx, group_sightings(nullptr, pk32, first, cnt, G));
  GroupCall a{nullptr, nullptr, pk32, sig64, first, cnt, msg32, out_group_bitmap, out_sig_bitmap};
  return verify_groups(ctx, a, G);
}

int nt_ed25519_verify_batch_groups_keyset(nt_ctx* ctx, const nt_keyset* ks, const uint32_t* key_idx,
                                          const uint8_t* sig64, const uint64_t* first,
                                          const uint32_t* cnt, const uint8_t* msg32, uint64_t G,
                                          uint8_t* out_group_bitmap, uint8_t* out_sig_bitmap) {
  if (!ctx || !ks || ks->ctx != ctx) return NT_EINVAL;
  if (G && (!first || !cnt || !msg32 || !out_group_bitmap)) return NT_EINVAL;
  if (G == 0) return NT_OK;
  uint64_t m = 0;
  for (uint64_t g = 0; g < G; ++g) m += cnt[g];
  if (small_verify(ctx, m, nt::kRouteKeyCache)) {
    if (m && (!key_idx || !sig64)) return NT_EINVAL;
    return host_groups(ctx, sig64, first, cnt, msg32, G, out_group_bitmap, out_sig_bitmap,
                       [&](uint64_t s, uint8_t A[32]) { return keyset_key(ks, NT_MODE_COFACTORLESS, key_idx[s], A); });
  }
  ctx->calls_gpu++;
  const KeyDev kd{ks->t.get(), ks->bits, ks->nkeys};
  GroupCall a{&kd, nullptr, (const uint8_t*)key_idx, sig64, first, cnt, msg32, out_group_bitmap, out_sig_bitmap};
  return verify_groups(ctx, a, G);
}

}  // extern "C"
