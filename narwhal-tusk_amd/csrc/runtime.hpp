// runtime.hpp -- the host runtime's internal types, shared by the C-ABI
// translation units (context.cpp, calibrate.cpp, verify.cpp, groups.cpp,
// keyset.cpp, sign.cpp, dev_api.cpp: one per family of entry points;
// registry.cpp: the key registry; ingest_gpu.cpp, wingest_gpu.cpp: the primary's
// and the worker's wire ingestion on the device).  Not part of the ABI.
//
// A context (nt_ctx) holds one Device per device entry; an entry holds extra
// execution slots (Devices too) that share its tables.  A slot's per-stream state
// is its two Lanes: every uncached verify launch goes through Device::verify_on
// and every key-cache launch through Device::keyset_on, which order the lane's
// scratch by its event.  Buffers (DevBuf / HostBuf) own their memory.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/ntcrypto.h"
#include "kernels.hpp"
#include "key_table.hpp"
#include "small_model.hpp"

struct nt_ctx;
namespace ntrt {
struct KeyReg;


#define NT_TRY(expr)                       \
  do {                                     \
    hipError_t _e = (expr);                \
    if (_e != hipSuccess) return NT_EHIP;  \
  } while (0)

#define NT_CHK0(expr)             \
  do {                            \
    int _rc = (expr);             \
    if (_rc != NT_OK) return _rc; \
  } while (0)

// A grow-only buffer in device memory (DevBuf) or pinned host memory (HostBuf) that owns its
// allocation: move-only, freed with the object.  ensure() keeps a buffer that is large enough
// and otherwise replaces it (the contents are lost) by one of at least 64 KB, rounded up to
// 4 KB; a failed allocation leaves it empty, returns NT_ENOMEM and clears HIP's sticky error.
template <bool kHost>
struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  Buf() = default;
  Buf(Buf&& o) noexcept { *this = std::move(o); }
  Buf& operator=(Buf&& o) noexcept {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    return *this;
  }
  ~Buf() { release(); }
  void release() {
    if (p) (void)(kHost ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  int ensure(size_t bytes) {
    if (bytes <= cap) return NT_OK;
    release();
    size_t want = std::max<size_t>(bytes, 1 << 16);
    want = (want + 4095) & ~(size_t)4095;
    if ((kHost ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want)) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return NT_ENOMEM;
    }
    cap = want;
    return NT_OK;
  }
  template <class T>
  T* as() const { return (T*)p; }
};
using DevBuf = Buf<false>;
using HostBuf = Buf<true>;

// nt_host_alloc registry: [base, base + bytes) of every live pinned buffer (context.cpp)
extern std::mutex g_pin_mu;
extern std::map<uintptr_t, uint64_t> g_pinned;
bool is_pinned(const void* p, uint64_t bytes);

enum { B_DATA, B_OFF, B_LEN, B_PK, B_SIG, B_OUT, B_OUT2, B_FIRST, B_CNT, B_NBUF };  // staging buffers of a slot

// The wide comb of B of one digit width on one device ordinal, shared by every
// device entry of every context of the process that runs on that ordinal at
// that width (11.8 GB at 24-bit digits, 872 MB at 20: round 2 paid it per entry
// -- repeated ordinals, a second Backend, the contention probe's contexts;
// ADVICE r02).  Built by the first verify / sign call that needs it (never at
// nt_init: a digest-only worker pays nothing), freed with the last user
// (context.cpp: shared_comb_b, comb_b_for).
struct CombB {
  int ordinal = -1;
  int bits = 0;
  uint32_t* p = nullptr;
  ~CombB() {
    if (!p) return;
    (void)hipSetDevice(ordinal);
    (void)hipFree(p);
  }
};
struct Device;
std::shared_ptr<CombB> shared_comb_b(Device& dv, int bits, int& rc);
// the comb of B of a slot (created by its entry on first use; context.cpp)
int comb_b_for(Device& dv);

// The context's HBM budget on one device entry (shared by its execution slots
// and by the key sets built on it): the TABLES whose width degrades to fit --
// the comb of B (24 -> 20 bits) and the committee key combs (20 -> 18 -> 16) --
// are reserved against `limit` (NT_HBM_BUDGET / nt_set_hbm_budget; 0 = no cap,
// only the device's free memory decides).  Workspaces, stashes and staging are
// per-call and not budgeted (nt_memory_info reports them).  The x cache (one fixed-size table
// per entry, no width to degrade) counts against the same limit in `aux`, beside the combs'
// `held` that nt_memory_info reports.
struct Budget {
  std::mutex mu;
  uint64_t limit = 0;
  uint64_t held = 0;
  uint64_t aux = 0;
  bool reserve(uint64_t b) {
    std::lock_guard<std::mutex> lk(mu);
    if (limit && held + aux + b > limit) return false;
    held += b;
    return true;
  }
  void release(uint64_t b) {
    std::lock_guard<std::mutex> lk(mu);
    held -= std::min(held, b);
  }
  bool reserve_aux(uint64_t b) {
    std::lock_guard<std::mutex> lk(mu);
    if (limit && held + aux + b > limit) return false;
    aux += b;
    return true;
  }
  void release_aux(uint64_t b) {
    std::lock_guard<std::mutex> lk(mu);
    aux -= std::min(aux, b);
  }
  bool fits(uint64_t b) {
    std::lock_guard<std::mutex> lk(mu);
    return !limit || held + aux + b <= limit;
  }
};

// The device entry's two compute streams.  Default: plain non-blocking
// streams (ordered against no other stream, the NULL stream included -- ADVICE
// r04: a CU-masked stream is a BLOCKING stream, so every launch on it waited
// for, and held up, work on the NULL stream of the whole process).  HIP
// multiplexes a process's streams over GPU_MAX_HW_QUEUES (4) queues per
// priority and hands a new stream the least-used one, so the two may share a
// hardware queue with other streams of the process; NT_STREAMS=mask gives each
// one a queue of its own (a CU mask enabling every CU: a masked stream never
// shares its queue) at the price of NULL-stream ordering, NT_STREAMS=prio puts
// the second at the highest priority.  Measured (profiles/r04/ab_streams.txt,
// profiles/r05/): the kinds give the same rates when the pipelined steps run on
// the library's streams.
inline hipError_t compute_stream(hipStream_t* s, uint32_t cus, int which) {
  static const int kind = [] {
    const char* e = std::getenv("NT_STREAMS");
    if (!e) return 1;
    return std::strcmp(e, "mask") == 0 ? 0 : std::strcmp(e, "prio") == 0 ? 2 : 1;
  }();
  if (kind == 1 || (kind == 2 && which == 0)) return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  if (kind == 2) {
    int lo = 0, hi = 0;
    const hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
    return e != hipSuccess ? e : hipStreamCreateWithPriority(s, hipStreamNonBlocking, hi);
  }
  std::vector<uint32_t> mask((cus + 31) / 32, 0xffffffffu);
  if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
  return hipExtStreamCreateWithCUMask(s, (uint32_t)mask.size(), mask.data());
}

// One compute stream of an execution slot and the scratch of the launches that alternate onto
// it: host chunk c runs on lane[c & 1], successive device-API calls take the lanes in turn
// (on the caller's stream).  Each buffer has an event that its every launch waits on and
// records, whatever stream the launch runs on, so two users of one buffer never overlap while
// the two lanes do.  Grow-only; nothing is allocated at nt_init.
struct Lane {
  hipStream_t stream = nullptr;
  DevBuf ws;          // [k]A workspace of the uncached verify kernel
  hipEvent_t ws_done = nullptr;
  DevBuf stash, sort;  // key-cache stash + key-grouping scratch (nt::KsScratch)
  hipEvent_t stash_done = nullptr;
};

struct Device {
  int ordinal = -1;
  int group = -1;               // index of this device entry in nt_ctx::devs (keyset tables)
  Device* entry = this;         // the device entry this execution slot belongs to
  std::shared_ptr<Budget> budget;  // the entry's (shared with its slots)
  std::mutex tables_mu;         // (entry) lazy creation of the comb of B
  std::shared_ptr<CombB> combB;  // holds d_combB (shared per ordinal and width, see CombB); null until first needed
  uint64_t comb_reserved = 0;   // (entry) bytes of the comb of B reserved in the budget
  uint32_t* d_combB = nullptr;  // wide comb of B (verify, key-cache verify, sign): comb_b_for() sets it
  int bbits = 0;                // its digit width (nt::kBCombBits or nt::kBCombFallback)
  std::atomic<int> comb_ready{0};  // this slot's d_combB / bbits are set (comb_b_for's lock-free fast path)
  // The x cache (ed25519_ops.hpp XCache): uint4 xtab[xslots][2], one table per device entry,
  // shared by its execution slots and both workspaces; xcache_for() (context.cpp) allocates it
  // zero-filled with the first verify and hands every slot the entry's pointer.  Null = none
  // (NT_XCACHE_SLOTS=0, or it did not fit the budget / the device).
  void* d_xtab = nullptr;
  uint32_t xslots = 0;          // a power of two
  uint64_t xtab_reserved = 0;   // (entry) its bytes in the budget
  bool xtab_tried = false;      // (entry) under tables_mu
  std::atomic<int> xtab_ready{0};  // this slot's d_xtab / xslots are set
  // The key-table cache (ktab.hpp): one per device entry, shared like the x cache;
  // ktab_for() (context.cpp) allocates it with the first verify -- the control block and the
  // index zero-filled, the pool as hipMalloc leaves it (a pool line is read only after a slot
  // names its entry) -- and never rewrites or frees an entry before the context closes.
  void* d_kslots = nullptr;     // the control block, then nt::kKTabIndexSlots slots of 8 bytes (nt::KTabArgs::base)
  void* d_kpool = nullptr;      // kcap entries of nt::ktab_entry_bytes()
  void* d_kext = nullptr;       // the second pool, kcap combs of nt::ktab_ext_bytes(): allocated, shared and freed with the pool
  uint32_t kcap = 0;
  uint64_t ktab_reserved = 0;   // (entry) its bytes in the budget
  bool ktab_tried = false;      // (entry) under tables_mu
  std::atomic<int> ktab_ready{0};  // this slot's d_kslots / d_kpool / kcap are set
  std::atomic<int> ktab_paused{0};  // (entry) > 0: launches carry no cache (calibrate_small's uncached floor)
  uint32_t ws_slots = 0;
  uint32_t sign_blocks = 0;
  uint32_t cus = 0;       // the CUs launches are sized for (NT_GRID_CUS; else real_cus)
  uint32_t real_cus = 0;  // the device's
  // host entry points: chunk c's H2D copies go on cstream, cev[c] marks them
  // done, and the host launches chunk c's kernels once it has waited for cev[c]
  // (pipeline.hpp run_chunks), so copies of chunk c+1 overlap kernels of chunk c
  hipStream_t cstream = nullptr;
  hipEvent_t cev[16] = {};
  // ... and chunks alternate between the two lanes, so the waves of chunk c+1
  // fill the CUs that chunk c's last waves leave idle.  Work that is not chunked
  // (table builds, read-backs, signing) runs on lane[0].stream.
  Lane lane[2];
  std::mutex mu;
  uint64_t dev_calls = 0;  // device-API verify calls (workspace alternation), under mu
  uint64_t ks_calls = 0;   // device-API key-cache calls (stash alternation), under mu
  DevBuf d[B_NBUF];
  HostBuf h[B_NBUF];
  // Extra execution slots of the same device entry (NT_SLOTS, default 2 in
  // all): each has its own streams, workspace and staging and shares the comb
  // of B, so a long call (a batch of digests) on one slot does not block a
  // concurrent call (a certificate batch) on the device -- both run on the GPU
  // at once.  Host entry points take the first free slot (SURVEY §8(b):
  // "per-call stream acquisition from a pool").
  std::vector<std::unique_ptr<Device>> extra;
  // state of the wire-ingestion entry point on this slot (ingest_gpu.cpp), created on first use
  std::shared_ptr<void> ingest;
  // ... and of the worker's (wingest_gpu.cpp)
  std::shared_ptr<void> wingest;

  // The buffers free themselves (after this body).  What needs an order: the streams drained
  // first, and the extra slots gone before this entry's comb of B and x table, which they borrow.
  ~Device() {
    if (comb_reserved && budget) budget->release(comb_reserved);
    if (xtab_reserved && budget) budget->release_aux(xtab_reserved);
    if (ktab_reserved && budget) budget->release_aux(ktab_reserved);
    if (ordinal < 0) return;
    (void)hipSetDevice(ordinal);
    for (Lane& l : lane)
      if (l.stream) (void)hipStreamSynchronize(l.stream);
    extra.clear();
    if (entry == this && d_xtab) (void)hipFree(d_xtab);
    if (entry == this && d_kslots) (void)hipFree(d_kslots);
    if (entry == this && d_kpool) (void)hipFree(d_kpool);
    if (entry == this && d_kext) (void)hipFree(d_kext);
    for (hipEvent_t e : {lane[0].ws_done, lane[0].stash_done, lane[1].ws_done, lane[1].stash_done})
      if (e) (void)hipEventDestroy(e);
    for (auto& e : cev)
      if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {cstream, lane[1].stream})
      if (s && s != lane[0].stream) (void)hipStreamDestroy(s);
    if (lane[0].stream) (void)hipStreamDestroy(lane[0].stream);
  }

  int init(int ord, int grp, Device* share = nullptr) {
    ordinal = ord;
    group = grp;
    entry = share ? share : this;
    budget = share ? share->budget : std::make_shared<Budget>();
    NT_TRY(hipSetDevice(ord));
    hipDeviceProp_t prop;
    NT_TRY(hipGetDeviceProperties(&prop, ord));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return NT_ENODEV;
    if (share) {
      // an extra (latency) slot: ONE stream at the highest priority for its
      // copies and kernels (both lanes share it; each keeps its own scratch),
      // so it does not share a hardware queue with the bulk streams of the
      // entry's first slot (HIP multiplexes a process's streams over
      // GPU_MAX_HW_QUEUES = 4 queues; a kernel behind a 17 ms digest flush in
      // the same queue waits for it)
      int lo = 0, hi = 0;
      NT_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
      NT_TRY(hipStreamCreateWithPriority(&lane[0].stream, hipStreamNonBlocking, hi));
      cstream = lane[1].stream = lane[0].stream;
    } else {
      // the two compute streams (compute_stream)
      NT_TRY(compute_stream(&lane[0].stream, (uint32_t)prop.multiProcessorCount, 0));
      NT_TRY(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
      NT_TRY(compute_stream(&lane[1].stream, (uint32_t)prop.multiProcessorCount, 1));
    }
    for (hipEvent_t* e : {&lane[0].ws_done, &lane[0].stash_done, &lane[1].ws_done, &lane[1].stash_done}) {
      NT_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
      NT_TRY(hipEventRecord(*e, lane[0].stream));
    }
    for (auto& e : cev) NT_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    // Nothing large is allocated here: the comb of B and the verify workspaces
    // come with the first call that needs them (comb_b_for, verify_tables, verify_on).
    // Workspace slots = grid cap of the verify kernel.  Four times the resident
    // workgroups (256-thread blocks, `occupancy` waves per SIMD, 4 SIMDs per CU):
    // up to 2M signatures per launch the grid is then one 512-signature block per
    // slot and the hardware dispatcher balances the tail (interleaved A/B on
    // MI355X, tools/ab_env.sh: ~1% over 1x and 2x resident).
    // NT_GRID_CUS=<n> (read by every context and slot): launches sized as for a device of n CUs,
    // 1 .. the real count -- the grid caps below and the `cus` the key-cache plans, their stash
    // bound and the host chunk rounds go by.  A batch then takes the passes of the grid-stride
    // loops that a CU partition, or a launch beyond a full device's grid, takes (tests).  The
    // CU-mask streams above and the clock probe keep the real count.
    real_cus = (uint32_t)prop.multiProcessorCount;
    cus = real_cus;
    if (const char* e = std::getenv("NT_GRID_CUS")) cus = (uint32_t)std::min<long>(std::max(1L, std::atol(e)), (long)real_cus);
    uint32_t slots = cus * (uint32_t)nt::verify_occupancy() * 4;
    if (const char* e = std::getenv("NT_WS_SLOTS")) slots = (uint32_t)std::max(1, std::atoi(e));
    ws_slots = slots;
    sign_blocks = cus * 8;
    NT_TRY(hipStreamSynchronize(lane[0].stream));
    return NT_OK;
  }

  // Wide combs of nkeys encoded points (host words) into d_comb (device);
  // negate: comb of -P (committee keys) instead of P (the base point).
  // s: the stream the build runs on (null = lane[0].stream; the key
  // registry's admissions pass a low-priority stream of their own)
  int build_wcombs(int bits, const uint32_t* enc_host, uint32_t nkeys, int negate, uint32_t* d_comb, uint32_t* d_meta,
                   hipStream_t s = nullptr) {
    if (nkeys == 0) return NT_OK;
    if (!s) s = lane[0].stream;
    const uint32_t batch = std::min<uint32_t>(nkeys, nt::wcomb_fill_batch(bits));
    uint32_t *d_enc = nullptr, *d_bases = nullptr, *d_tmp = nullptr;
    int rc = NT_OK;
    if (hipMalloc(&d_enc, 32ull * nkeys) != hipSuccess ||
        hipMalloc(&d_bases, nt::wcomb_bases_bytes_per_key(bits) * nkeys) != hipSuccess ||
        hipMalloc(&d_tmp, nt::wcomb_fill_tmp_bytes_per_key(bits) * batch) != hipSuccess) {
      rc = NT_ENOMEM;
    } else if (hipMemcpyAsync(d_enc, enc_host, 32ull * nkeys, hipMemcpyHostToDevice, s) != hipSuccess ||
               nt::launch_wcomb_build(bits, d_enc, nkeys, negate, d_comb, d_meta, d_bases, d_tmp, batch, s) !=
                   hipSuccess ||
               hipStreamSynchronize(s) != hipSuccess) {
      rc = NT_EHIP;
    }
    if (d_enc) (void)hipFree(d_enc);
    if (d_bases) (void)hipFree(d_bases);
    if (d_tmp) (void)hipFree(d_tmp);
    return rc;
  }

  // The x cache as a launch sees it.  NT_XCACHE_SLOTS is read again at every launch: a value
  // below the allocated size confines the launch to the table's first slots (0: no cache for
  // this launch), a larger one changes nothing.
  nt::XTab xtab() const {
    nt::XTab xt;
    if (!d_xtab) return xt;
    uint32_t slots = xslots;
    if (const char* e = std::getenv("NT_XCACHE_SLOTS")) slots = nt::xcache_slots_pow2(std::strtoull(e, nullptr, 10), xslots);
    if (slots) {
      xt.tab = d_xtab;
      xt.mask = slots - 1;
    }
    return xt;
  }

  // The key-table cache as a launch sees it.  NT_KTAB_KEYS is read again at every launch: 0 = no
  // cache for this launch, a value below the allocated capacity confines the launch to the pool's
  // first entries (entries beyond it are misses, none is added), a larger one changes nothing.
  nt::KTabArgs ktab() const {
    nt::KTabArgs kt;
    if (!d_kslots || !d_kpool || !d_kext || entry->ktab_paused.load(std::memory_order_relaxed)) return kt;
    uint32_t cap = kcap;
    if (const char* e = std::getenv("NT_KTAB_KEYS")) cap = (uint32_t)std::min<unsigned long long>(std::strtoull(e, nullptr, 10), kcap);
    if (cap) {
      kt.base = d_kslots;
      kt.cap = cap;
    }
    return kt;
  }

  // compute stream of chunk c
  hipStream_t cstr(int c) const { return lane[c & 1].stream; }

  // Grow a buffer that an earlier enqueue-only (device-API) call may still be
  // using: wait for its last user (the launch that recorded ev) before freeing it.
  static int grow_synced(DevBuf& b, size_t bytes, hipEvent_t ev) {
    if (bytes <= b.cap) return NT_OK;
    if (b.p && hipEventSynchronize(ev) != hipSuccess) return NT_EHIP;
    return b.ensure(bytes);
  }

  // Uncached verify launch on stream s with lane l's [k]A workspace, grown to `slots` workspace
  // slots (ws_slots x 737 KB is ~1.5 GB at 2,048 slots) and ordered against the workspace's
  // other users by its event; per_lane as in nt::launch_verify.  A device-API caller (s its own
  // stream) holds mu.
  int verify_on(Lane& l, hipStream_t s, int mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                uint64_t msg_bytes, const uint64_t* off, const uint64_t* len, uint64_t n, uint64_t* out, int per_lane,
                uint64_t slots) {
    slots = std::max<uint64_t>(slots, 1);
    NT_CHK0(grow_synced(l.ws, nt::ws_bytes_per_slot() * slots, l.ws_done));
    if (hipStreamWaitEvent(s, l.ws_done, 0) != hipSuccess ||
        nt::launch_verify(mode, pk, sig, msg, msg_bytes, off, len, n, d_combB, bbits, l.ws.p, (uint32_t)slots, out, s,
                          per_lane, xtab(), ktab()) != hipSuccess ||
        hipEventRecord(l.ws_done, s) != hipSuccess)
      return NT_EHIP;
    return NT_OK;
  }
  // ... of host chunk c, on its lane's stream.  Workspace sizes: lane 0's holds ws_slots slots
  // from the slot's first verify on (verify_tables; ws_bytes_per_slot() is a multiple of 4,096,
  // so the DevBuf holds exactly that), lane 1's grows to the largest grid a chunk launched
  // (device-API calls grow either lane's to ws_slots).
  int verify_host(size_t c, int mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint64_t msg_bytes,
                  const uint64_t* off, const uint64_t* len, uint64_t n, uint64_t* out, int per_lane = 0) {
    Lane& l = lane[c & 1];
    return verify_on(l, l.stream, mode, pk, sig, msg, msg_bytes, off, len, n, out, per_lane,
                     (c & 1) ? nt::verify_grid(n, ws_slots, per_lane) : ws_slots);
  }

  // lane l's key-cache scratch holds launches of up to max_sigs signatures
  int ensure_scratch(Lane& l, uint64_t max_sigs) {
    NT_CHK0(grow_synced(l.stash, nt::keyset_stash_bytes(max_sigs, cus), l.stash_done));
    return grow_synced(l.sort, nt::keyset_sort_bytes(max_sigs), l.stash_done);
  }
  // Key-cache launch on stream s with lane l's scratch: launch(nt::KsScratch) enqueues it on s,
  // after the scratch's previous user (host chunks on the lanes' streams, device-API calls on
  // any stream) and before its next, like verify_on's workspace.
  template <class F>
  int keyset_on(Lane& l, hipStream_t s, uint64_t max_sigs, F&& launch) {
    NT_CHK0(ensure_scratch(l, max_sigs));
    if (hipStreamWaitEvent(s, l.stash_done, 0) != hipSuccess ||
        launch(nt::KsScratch{l.stash.p, l.sort.p}) != hipSuccess || hipEventRecord(l.stash_done, s) != hipSuccess)
      return NT_EHIP;
    return NT_OK;
  }
};

}  // namespace ntrt

struct nt_ctx {
  std::vector<std::unique_ptr<ntrt::Device>> devs;
  uint64_t hbm_budget = 0;   // per device entry (Budget::limit); NT_HBM_BUDGET at init
  NtSmallModel small_model;  // written by nt_set_small_call_path before small_mode
  // small-call path (cpu_lane.hpp): NT_SMALL_OFF / AUTO / ALWAYS, host threads
  std::atomic<int> small_mode{NT_SMALL_OFF};
  std::atomic<int> small_threads{1};
  std::atomic<uint64_t> calls_host{0}, calls_gpu{0};
  // the key registry (nt_set_key_cache; registry.cpp): declared after devs so
  // that it -- its admission thread and device tables -- goes first
  std::shared_ptr<ntrt::KeyReg> reg;
};

namespace ntrt {
// Device tables of a key set, shared by its nt_keyset handle and every
// nt_committee built on it: a committee keeps them alive, so freeing the key set
// before the committee is safe.  The key combs' bytes are reserved
// in each device entry's budget while the tables live.
struct KsTables {
  uint32_t nkeys = 0;
  int bits = 0;                 // comb digit width of every key (nt::kKeyComb{Wide,Mid,Narrow})
  struct PerDev {
    int ordinal = -1;
    uint32_t* d_enc = nullptr;
    uint32_t* d_meta = nullptr;
    uint32_t* d_comb = nullptr;
    std::shared_ptr<Budget> budget;
    uint64_t reserved = 0;
  };
  std::vector<PerDev> dev;
  ~KsTables() {
    for (auto& d : dev) {
      if (d.budget && d.reserved) d.budget->release(d.reserved);
      if (d.ordinal < 0) continue;
      (void)hipSetDevice(d.ordinal);
      if (d.d_enc) (void)hipFree(d.d_enc);
      if (d.d_meta) (void)hipFree(d.d_meta);
      if (d.d_comb) (void)hipFree(d.d_comb);
    }
  }
};

// The device tables one key-cache launch reads: a key set's, or a published
// snapshot of the key registry's (keys >= nkeys verify as unknown -> reject).
struct KeyDev {
  const KsTables* t = nullptr;
  int bits = 0;
  uint32_t nkeys = 0;
};
// What a key-cache launch on slot dv reads: the first nkeys keys of pd's tables (a key set's,
// a registry snapshot's or a committee's share on dv's entry) at `bits`-bit digits, and the
// slot's comb of B (comb_b_for(dv) has run).
inline nt::KsTabs ks_tabs(const KsTables::PerDev& pd, int bits, uint32_t nkeys, const Device& dv) {
  return nt::KsTabs{bits, pd.d_meta, pd.d_enc, pd.d_comb, nkeys, dv.d_combB, dv.bbits, dv.cus};
}

// A published state of the key registry (registry.cpp): the host index of
// keys 0 .. table.nkeys - 1 and the device tables that hold their combs
// (allocated for `capacity` keys at the first admission; entries below
// table.nkeys are never written again, so a call that holds this snapshot
// reads them while later admissions fill the entries above).
struct RegSnap {
  nt::KeyTable table;
  std::shared_ptr<KsTables> t;
  int bits = 0;
  KeyDev dev() const { return KeyDev{t.get(), bits, table.nkeys}; }
};
// the published snapshot of ctx's registry, or null (registry off / empty)
std::shared_ptr<const RegSnap> reg_snapshot(nt_ctx* ctx);
// keys a call could not find: up to kRegNoteMax distinct ones are counted as
// sightings (and queued for admission once seen `admit_after` times)
constexpr uint32_t kRegNoteMax = 256;
void reg_note_misses(nt_ctx* ctx, const std::vector<const uint8_t*>& keys);
void reg_count(nt_ctx* ctx, uint64_t hits, uint64_t misses);
// first-use tables and width choice shared with nt_keyset_create (context.cpp)
int keyset_comb_bits(nt_ctx* ctx, uint32_t nkeys);
hipError_t table_malloc(void** p, size_t bytes);  // comb tables (NT_TABLE_ALLOC)
int comb_b_for(Device& dv);

}  // namespace ntrt

struct nt_keyset {
  nt_ctx* ctx = nullptr;
  uint32_t nkeys = 0;
  std::vector<uint8_t> enc;     // host copy of the key encodings (small-call path)
  int bits = 0;                 // = t->bits
  std::vector<uint32_t> flags;  // host copy of kKey* bits
  std::shared_ptr<ntrt::KsTables> t;
};

namespace ntrt {

// Split [0, n) into one contiguous range per device, boundaries multiple of `align`.
inline std::vector<std::pair<uint64_t, uint64_t>> shard(uint64_t n, size_t ndev, uint64_t align) {
  std::vector<std::pair<uint64_t, uint64_t>> r;
  uint64_t per = (n + ndev - 1) / ndev;
  per = (per + align - 1) / align * align;
  uint64_t lo = 0;
  for (size_t d = 0; d < ndev; ++d) {
    const uint64_t hi = std::min(n, lo + per);
    r.emplace_back(lo, hi);
    lo = hi;
  }
  return r;
}

// The execution slot of device entry d a call runs on, locked into lk.  Bulk
// calls take the entry's own slot (waiting for it), so the extra
// high-priority slots stay free for latency-sized calls; a latency-sized call
// takes the first free extra slot, else the entry's own slot if free, else
// waits for the first extra slot (two concurrent bulk calls must
// not occupy both slots and block a certificate-sized call behind a digest).
inline Device& acquire_slot(nt_ctx* ctx, size_t d, bool latency, std::unique_lock<std::mutex>& lk) {
  Device& p = *ctx->devs[d];
  if (!latency || p.extra.empty()) {
    lk = std::unique_lock<std::mutex>(p.mu);
    return p;
  }
  std::vector<Device*> order;
  for (auto& x : p.extra) order.push_back(x.get());
  order.push_back(&p);
  for (Device* s : order) {
    std::unique_lock<std::mutex> l(s->mu, std::try_to_lock);
    if (l.owns_lock()) {
      lk = std::move(l);
      return *s;
    }
  }
  lk = std::unique_lock<std::mutex>(order[0]->mu);
  return *order[0];
}

// digests whose longest message is short (header / vote / certificate
// preimages) finish fast; long ones (worker batches) are bulk
inline bool sha_latency(uint64_t n, const uint64_t* len) {
  for (uint64_t i = 0; i < n; ++i)
    if (len[i] > (64u << 10)) return false;
  return true;
}

// work below one round of resident waves: a latency-sized call
inline bool latency_sized(const nt_ctx* ctx, uint64_t items_per_device, uint64_t round) {
  (void)ctx;
  return items_per_device <= round;
}

template <class F>
int run_sharded(nt_ctx* ctx, uint64_t n, uint64_t align, F&& fn, bool latency = false) {
  const size_t nd = ctx->devs.size();
  auto parts = shard(n, nd, align);
  if (nd == 1) {
    std::unique_lock<std::mutex> lk;
    Device& dv = acquire_slot(ctx, 0, latency, lk);
    if (hipSetDevice(dv.ordinal) != hipSuccess) return NT_EHIP;
    return fn(dv, parts[0].first, parts[0].second);
  }
  std::vector<int> rcs(nd, NT_OK);
  std::vector<std::thread> th;
  for (size_t d = 0; d < nd; ++d) {
    if (parts[d].first >= parts[d].second) continue;
    th.emplace_back([&, d] {
      std::unique_lock<std::mutex> lk;
      Device& dv = acquire_slot(ctx, d, latency, lk);
      if (hipSetDevice(dv.ordinal) != hipSuccess) {
        rcs[d] = NT_EHIP;
        return;
      }
      rcs[d] = fn(dv, parts[d].first, parts[d].second);
    });
  }
  for (auto& t : th) t.join();
  for (int rc : rcs)
    if (rc != NT_OK) return rc;
  return NT_OK;
}

#define NT_CHK(expr)              \
  do {                            \
    int _rc = (expr);             \
    if (_rc != NT_OK) return _rc; \
  } while (0)

// ---- what the translation units share besides the types above ----
// context.cpp: everything the verify kernel of slot dv reads besides its inputs; device entry `dev` or null
int verify_tables(Device& dv);
Device* dev_of(nt_ctx* ctx, int dev);
// context.cpp, the small-call path (cpu_lane.hpp): NT_SMALL_* overrides of single
// model fields, the host threads of a call of `items` items, and whether the host lane takes
// a verify call (kind: nt::kRouteUncached / kRouteKeyCache) or a digest call
NtSmallModel small_model_with_env(NtSmallModel m);
int small_threads(const nt_ctx* ctx, uint64_t items);
bool small_verify(nt_ctx* ctx, uint64_t nsig, int kind = nt::kRouteUncached);
bool small_sha(nt_ctx* ctx, uint64_t n, const uint64_t* len);
int calibrate_small(nt_ctx* ctx);  // calibrate.cpp
// verify.cpp: the GPU bodies of nt_ed25519_verify_strict (no registry) and nt_ed25519_verify_keyset
int verify_strict_gpu(nt_ctx* ctx, const uint8_t* pk32, const uint8_t* sig64, const uint8_t* msg, const uint64_t* off,
                      const uint64_t* len, uint64_t n, uint8_t* out_bitmap);
int verify_keyset_gpu(nt_ctx* ctx, const KeyDev& kd, int mode, const uint32_t* key_idx, const uint8_t* sig64,
                      const uint8_t* msg, const uint64_t* off, const uint64_t* len, uint64_t n, uint8_t* out_bitmap);
// keyset.cpp: nt_keyset_create at a given key-comb width (0 = the widest that fits); the key
// encoding and check mode of one key-cache entry on the small-call path (-1: no such key)
int keyset_create(nt_ctx* ctx, const uint8_t* pk32, uint32_t nkeys, int bits, nt_keyset** out);
int keyset_key(const nt_keyset* ks, int mode, uint32_t kraw, uint8_t A[32]);


}  // namespace ntrt
