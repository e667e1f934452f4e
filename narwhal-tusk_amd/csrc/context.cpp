// context.cpp -- host side of the C ABI (include/ntcrypto.h): contexts, memory,
// tables and the small-call setters; the other entry points live in verify.cpp,
// groups.cpp, keyset.cpp, sign.cpp and dev_api.cpp, all over runtime.hpp.
//
// Owns one `Device` per GPU (per entry of nt_init_devices: a repeated ordinal
// gets its own): non-blocking HIP streams and grow-only device/pinned staging;
// on the first call that needs them, the wide comb of B (24-bit digits, 11.8 GB,
// shared per device ordinal; 20-bit, 872 MB, under an HBM budget or when the
// device cannot hold the wide one) and the per-lane [k]A table workspace.
// Host entry points shard items over devices by contiguous index ranges (one
// host thread per device), stage through pinned memory, launch, and gather the
// bitmaps / digests.  There is deliberately no CPU compute path: if HIP or the
// gfx950 code object is unavailable the call fails with a negative code.
#include <cmath>

#include "cpu_lane.hpp"
#include "runtime.hpp"

namespace ntrt {

// NT_TABLE_ALLOC=contig (A/B): comb tables from physically contiguous VRAM
// (hipExtMallocWithFlags + hipDeviceMallocContiguous; hipMalloc when that is
// refused), to see whether the key-cache kernel's random comb lines pay for
// address translation beyond what the driver's own placement gives
hipError_t table_malloc(void** p, size_t bytes) {
  static const bool contig = [] {
    const char* e = std::getenv("NT_TABLE_ALLOC");
    return e && std::strcmp(e, "contig") == 0;
  }();
  if (contig) {
    const hipError_t e = hipExtMallocWithFlags(p, bytes, hipDeviceMallocContiguous);
    if (std::getenv("NT_REG_TRACE"))
      std::fprintf(stderr, "[alloc] contiguous %.2f GB: %s\n", bytes / 1e9, e == hipSuccess ? "ok" : "refused");
    if (e == hipSuccess) return e;
    (void)hipGetLastError();
  }
  return hipMalloc(p, bytes);
}

// nt_host_alloc registry (runtime.hpp)
std::mutex g_pin_mu;
std::map<uintptr_t, uint64_t> g_pinned;

bool is_pinned(const void* p, uint64_t bytes) {
  std::lock_guard<std::mutex> lk(g_pin_mu);
  auto it = g_pinned.upper_bound((uintptr_t)p);
  if (it == g_pinned.begin()) return false;
  --it;
  return (uintptr_t)p + bytes <= it->first + it->second;
}

// comb of B per (device ordinal, digit width), shared across device entries and contexts
std::mutex g_combb_mu;
std::map<std::pair<int, int>, std::weak_ptr<CombB>> g_combb;

std::shared_ptr<CombB> shared_comb_b(Device& dv, int bits, int& rc) {
  static const uint32_t kB[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                                 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};  // encoding of B
  std::lock_guard<std::mutex> lk(g_combb_mu);
  if (auto c = g_combb[{dv.ordinal, bits}].lock()) return c;
  auto c = std::make_shared<CombB>();
  c->ordinal = dv.ordinal;
  c->bits = bits;
  if (hipSetDevice(dv.ordinal) != hipSuccess) {
    rc = NT_EHIP;
    return nullptr;
  }
  if (table_malloc((void**)&c->p, nt::wcomb_bytes_per_key(bits)) != hipSuccess) {
    (void)hipGetLastError();  // an out-of-memory hipMalloc leaves no sticky error: clear it
    c->p = nullptr;
    rc = NT_ENOMEM;
    return nullptr;
  }
  rc = dv.build_wcombs(bits, kB, 1, 0, c->p, nullptr);
  if (rc != NT_OK) return nullptr;
  g_combb[{dv.ordinal, bits}] = c;
  return c;
}

// NT_BCOMB_BITS=24|20 forces the width of the comb of B (A/B runs, tests)
static int forced_bcomb_bits() {
  const char* e = std::getenv("NT_BCOMB_BITS");
  const int b = e ? std::atoi(e) : 0;
  return b == nt::kBCombBits || b == nt::kBCombFallback ? b : 0;
}

// HBM the device must keep free beside a 24-bit comb of B (two slots' verify
// workspaces + staging); below it the entry takes the 20-bit comb
constexpr uint64_t kCombHeadroom = 4ull << 30;

// The comb of B of execution slot dv: its entry's, created on first use.  The
// entry picks the widest width that (a) fits the context's HBM budget on the
// entry, (b) leaves kCombHeadroom of the device free and (c) hipMalloc grants:
// 24-bit digits (11 additions per [s]B, 11.8 GB), else 20-bit (13, 872 MB).
// The fast path reads only the slot's own comb_ready (the entry's
// fields are written under tables_mu by whichever slot builds the comb first).
int comb_b_for(Device& dv) {
  if (dv.comb_ready.load(std::memory_order_acquire)) return NT_OK;
  Device& e = *dv.entry;
  std::lock_guard<std::mutex> lk(e.tables_mu);
  if (!e.combB) {
    const int forced = forced_bcomb_bits();
    int rc = NT_ENOMEM;
    for (const int w : {nt::kBCombBits, nt::kBCombFallback}) {
      if (forced && w != forced) continue;
      const uint64_t bytes = nt::wcomb_bytes_per_key(w);
      if (!forced && w == nt::kBCombBits) {
        size_t fr = 0, tot = 0;
        if (hipSetDevice(e.ordinal) != hipSuccess || hipMemGetInfo(&fr, &tot) != hipSuccess) return NT_EHIP;
        // an existing comb of this width on the ordinal costs nothing more
        std::shared_ptr<CombB> have;
        {
          std::lock_guard<std::mutex> g(g_combb_mu);
          auto it = g_combb.find({e.ordinal, w});
          if (it != g_combb.end()) have = it->second.lock();
        }
        if (!have && fr < bytes + kCombHeadroom) continue;
      }
      if (!e.budget->reserve(bytes)) continue;
      auto c = shared_comb_b(e, w, rc);
      if (!c) {
        e.budget->release(bytes);
        if (rc != NT_ENOMEM) return rc;
        continue;
      }
      e.combB = c;
      e.d_combB = c->p;
      e.bbits = w;
      e.comb_reserved = bytes;
      rc = NT_OK;
      break;
    }
    if (rc != NT_OK) return rc;
  }
  dv.combB = e.combB;
  dv.d_combB = e.d_combB;
  dv.bbits = e.bbits;
  dv.comb_ready.store(1, std::memory_order_release);
  return NT_OK;
}

// The x cache of execution slot dv: its entry's, allocated by the entry's first verify that finds
// NT_XCACHE_SLOTS non-zero, at that many slots (default 2^21 = 64 MB; rounded down to a power of two),
// zero-filled, and reserved in the entry's HBM budget.  A table that does not fit the budget or
// the device is skipped silently: the kernel then decompresses every key as before.
static void xcache_for(Device& dv) {
  if (dv.xtab_ready.load(std::memory_order_acquire)) return;
  Device& e = *dv.entry;
  std::lock_guard<std::mutex> lk(e.tables_mu);
  if (!e.xtab_tried) {
    unsigned long long want = nt::kXCacheSlotsDefault;
    if (const char* v = std::getenv("NT_XCACHE_SLOTS")) want = std::strtoull(v, nullptr, 10);
    const uint32_t slots = nt::xcache_slots_pow2(want, nt::kXCacheSlotsMax);
    if (!slots) return;  // off for this launch: the first one that asks for a table allocates it
    e.xtab_tried = true;
    const uint64_t bytes = 32ull * slots;
    if (e.budget->reserve_aux(bytes)) {
      void* p = nullptr;
      hipStream_t s = dv.lane[0].stream;
      if (hipSetDevice(e.ordinal) == hipSuccess && hipMalloc(&p, bytes) == hipSuccess &&
          hipMemsetAsync(p, 0, bytes, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess) {
        e.d_xtab = p;
        e.xslots = slots;
        e.xtab_reserved = bytes;
      } else {
        (void)hipGetLastError();
        if (p) (void)hipFree(p);
        e.budget->release_aux(bytes);
      }
    }
  }
  if (&dv != &e) {
    dv.d_xtab = e.d_xtab;
    dv.xslots = e.xslots;
  }
  dv.xtab_ready.store(1, std::memory_order_release);
}

// The key-table cache of execution slot dv: its entry's, allocated by the entry's first verify that
// finds NT_KTAB_KEYS non-zero -- after the comb of B and the x cache -- at that many pool entries
// (default 2^20 = 4.16 GB, and 4.43 GB of second pool: the keys' combs, 4,224 B each -- 8,192 B per
// key, 8.6 GB in all; a -DNT_KCOMB=0 build keeps fourth tables there, 1,280 B each -- one unit with
// the pool: reserved, halved, freed and reported together) beside an index of 2^21 slots (16 MB) and
// the control block, both zero-filled, and reserved in the entry's HBM budget.  The default halves down to 2^14 entries
// while the budget (the cache keeps to 1/16 of a finite one: the rest is the combs') or the device
// (the comb's rule: 4 GB stay free) does not allow it; a size asked
// for by NT_KTAB_KEYS is tried as it is.  A cache that fits nowhere is skipped silently: the
// kernel then runs every verification on the balanced path as before.
// words 4..6 and 8..9 of the control block: the pool's address, the index mask and the second
// pool's address (read by every launch)
static hipError_t ktab_describe(void* base, void* pool, void* ext) {
  uint32_t w[6] = {};
  const uint64_t a = (uint64_t)(uintptr_t)pool, x = (uint64_t)(uintptr_t)ext;
  w[0] = (uint32_t)a;
  w[1] = (uint32_t)(a >> 32);
  w[2] = nt::kKTabIndexSlots - 1;
  w[4] = (uint32_t)x;
  w[5] = (uint32_t)(x >> 32);
  return hipMemcpy((uint8_t*)base + 16, w, sizeof w, hipMemcpyHostToDevice);
}
static void ktab_for(Device& dv) {
  if (dv.ktab_ready.load(std::memory_order_acquire)) return;
  Device& e = *dv.entry;
  std::lock_guard<std::mutex> lk(e.tables_mu);
  if (!e.ktab_tried) {
    unsigned long long want = nt::kKTabKeysDefault;
    const char* v = std::getenv("NT_KTAB_KEYS");
    if (v) want = std::min<unsigned long long>(std::strtoull(v, nullptr, 10), 1ull << 26);
    if (!want) return;  // off for this launch: the first one that asks for a cache allocates it
    e.ktab_tried = true;
    const uint64_t index_bytes = nt::kKTabCtlBytes + 8ull * nt::kKTabIndexSlots;
    hipStream_t s = dv.lane[0].stream;
    // Under a budget the cache keeps to 1/16 of it: what the budget leaves after the comb of B is
    // the key combs', whose width decides the rate of every key-cache launch.
    uint64_t share = ~0ull;
    {
      std::lock_guard<std::mutex> g(e.budget->mu);
      if (e.budget->limit) share = e.budget->limit / 16;
    }
    for (uint64_t keys = want; keys >= 1; keys /= 2) {
      const uint64_t bytes = index_bytes + keys * (nt::ktab_entry_bytes() + nt::ktab_ext_bytes());
      size_t fr = 0, tot = 0;
      if (hipSetDevice(e.ordinal) != hipSuccess || hipMemGetInfo(&fr, &tot) != hipSuccess) break;
      if (bytes <= share && fr >= bytes + kCombHeadroom && e.budget->reserve_aux(bytes)) {
        void *ps = nullptr, *pp = nullptr, *px = nullptr;
        if (hipMalloc(&ps, index_bytes) == hipSuccess && hipMalloc(&pp, keys * nt::ktab_entry_bytes()) == hipSuccess &&
            hipMalloc(&px, keys * nt::ktab_ext_bytes()) == hipSuccess &&
            hipMemsetAsync(ps, 0, index_bytes, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess &&
            ktab_describe(ps, pp, px) == hipSuccess) {
          e.d_kslots = ps;
          e.d_kpool = pp;
          e.d_kext = px;
          e.kcap = (uint32_t)keys;
          e.ktab_reserved = bytes;
          break;
        }
        (void)hipGetLastError();
        if (ps) (void)hipFree(ps);
        if (pp) (void)hipFree(pp);
        if (px) (void)hipFree(px);
        e.budget->release_aux(bytes);
      }
      if (v || keys / 2 < nt::kKTabKeysFloor) break;
    }
  }
  if (&dv != &e) {
    dv.d_kslots = e.d_kslots;
    dv.d_kpool = e.d_kpool;
    dv.d_kext = e.d_kext;
    dv.kcap = e.kcap;
  }
  dv.ktab_ready.store(1, std::memory_order_release);
}

// everything the verify kernel of slot dv reads besides its inputs; lane 0's [k]A workspace at
// its full ws_slots slots (before a call's copies start, not at its first launch)
int verify_tables(Device& dv) {
  NT_CHK(comb_b_for(dv));
  xcache_for(dv);
  ktab_for(dv);
  return Device::grow_synced(dv.lane[0].ws, nt::ws_bytes_per_slot() * dv.ws_slots, dv.lane[0].ws_done);
}

// Comb width of a new key set: the widest of 21 (reduced scalars) / 20 / 18 /
// 16-bit digits (12 / 13 / 15 / 16 additions per [k]A; 1.61 GB / 872 / 252 /
// 67 MB per key) that, on every device entry of the context, fits the
// context's HBM budget beside the comb of B and the tables the entry already
// holds, and leaves 1/8 of the device's HBM free.  With no width passing the
// free-memory test the 16-bit combs are tried anyway (hipMalloc decides); 0 =
// not even those fit the budget.  NT_KEYSET_COMB_BITS=16|18|20|21 forces one.
int keyset_comb_bits(nt_ctx* ctx, uint32_t nkeys) {
  if (const char* e = std::getenv("NT_KEYSET_COMB_BITS")) {
    const int b = std::atoi(e);
    if (b == nt::kKeyCombReduced || b == nt::kKeyCombWide || b == nt::kKeyCombMid || b == nt::kKeyCombNarrow)
      return b;
  }
  const uint64_t nk = std::max<uint32_t>(nkeys, 1);
  for (const int w : {nt::kKeyCombReduced, nt::kKeyCombWide, nt::kKeyCombMid, nt::kKeyCombNarrow}) {
    const uint64_t comb = nt::wcomb_bytes_per_key(w) * nk;
    const uint64_t need = comb + nt::wcomb_fill_tmp_bytes_per_key(w) * nt::wcomb_fill_batch(w);
    bool ok = true;
    for (auto& d : ctx->devs) {
      size_t fr = 0, tot = 0;
      if (!d->budget->fits(comb) || hipSetDevice(d->ordinal) != hipSuccess ||
          hipMemGetInfo(&fr, &tot) != hipSuccess || fr < need + tot / 8) {
        ok = false;
        break;
      }
    }
    if (ok) return w;
  }
  for (auto& d : ctx->devs)
    if (!d->budget->fits(nt::wcomb_bytes_per_key(nt::kKeyCombNarrow) * nk)) return 0;
  return nt::kKeyCombNarrow;
}

Device* dev_of(nt_ctx* ctx, int dev) {
  if (!ctx || dev < 0 || dev >= (int)ctx->devs.size()) return nullptr;
  return ctx->devs[dev].get();
}

// ---- small-call path (cpu_lane.hpp) -----------------------------
// Cost model of one host entry-point call (NtSmallModel, runtime.hpp).  A GPU
// call below one round of resident waves costs a fixed floor (launch + copies
// + the two signatures every lane of the verify kernel runs); the digest
// kernel's time is set by its LONGEST message (one lane's serial chain) plus
// the PCIe copy.  nt_set_small_call_path calibrates the fields on the
// context's host threads and device (calibrate.cpp); NT_SMALL_*
// environment variables override single fields (A/B runs).
int small_threads(const nt_ctx* ctx, uint64_t items) {
  const uint64_t t = (uint64_t)std::max(1, ctx->small_threads.load());
  return (int)std::max<uint64_t>(1, std::min(t, items));
}

// host lane iff the call's estimated host time on the context's threads is
// below the GPU floor of the kernel it would run (small_model.hpp)
bool small_verify(nt_ctx* ctx, uint64_t nsig, int kind) {
  const int mode = ctx->small_mode.load();
  if (mode == NT_SMALL_ALWAYS) return true;
  if (mode != NT_SMALL_AUTO || !nt::cpu::ready()) return false;
  return nt::small_verify_on_host(ctx->small_model, nsig, small_threads(ctx, nsig), kind);
}

bool small_sha(nt_ctx* ctx, uint64_t n, const uint64_t* len) {
  const int mode = ctx->small_mode.load();
  if (mode == NT_SMALL_ALWAYS) return true;
  if (mode != NT_SMALL_AUTO) return false;
  uint64_t total = 0, mx = 0;
  for (uint64_t i = 0; i < n; ++i) {
    total += len[i];
    mx = std::max(mx, len[i]);
  }
  return nt::small_sha_on_host(ctx->small_model, n, total, mx, small_threads(ctx, n));
}

static double env_or(const char* name, double dflt) {
  const char* e = std::getenv(name);
  return e && *e ? std::atof(e) : dflt;
}
NtSmallModel small_model_with_env(NtSmallModel m) {
  m.cpu_verify_us = env_or("NT_SMALL_CPU_VERIFY_US", m.cpu_verify_us);
  m.gpu_verify_us = env_or("NT_SMALL_GPU_VERIFY_US", m.gpu_verify_us);
  m.cpu_sha_mbs = env_or("NT_SMALL_CPU_SHA_MBS", m.cpu_sha_mbs);
  m.gpu_lane_mbs = env_or("NT_SMALL_GPU_LANE_MBS", m.gpu_lane_mbs);
  m.gpu_call_us = env_or("NT_SMALL_GPU_CALL_US", m.gpu_call_us);
  m.pcie_gbs = env_or("NT_SMALL_PCIE_GBS", m.pcie_gbs);
  m.spawn_us = env_or("NT_SMALL_SPAWN_US", m.spawn_us);
  m.gpu_keyset_us = env_or("NT_SMALL_GPU_KEYSET_US", m.gpu_keyset_us);
  return m;
}

}  // namespace ntrt

using namespace ntrt;

extern "C" {

const char* nt_strerror(int code) {
  switch (code) {
    case NT_OK: return "ok";
    case NT_EINVAL: return "invalid argument";
    case NT_EHIP: return "HIP runtime error";
    case NT_ENOMEM: return "out of device or pinned memory";
    case NT_ENODEV: return "no usable gfx950 device (this library has no CPU path)";
    default: return "unknown error";
  }
}

const char* nt_version(void) { return "ntcrypto 0.1 gfx950"; }

static long env_slots() {
  const char* e = std::getenv("NT_SLOTS");
  return e && *e ? std::atol(e) : 2;
}

// NT_HBM_BUDGET: bytes of tables per device entry, with an optional K / M / G suffix (0 / unset = no cap)
static uint64_t env_budget() {
  const char* e = std::getenv("NT_HBM_BUDGET");
  if (!e || !*e) return 0;
  char* end = nullptr;
  const double v = std::strtod(e, &end);
  double mul = 1;
  if (end && (*end == 'k' || *end == 'K')) mul = 1024.0;
  if (end && (*end == 'm' || *end == 'M')) mul = 1024.0 * 1024;
  if (end && (*end == 'g' || *end == 'G')) mul = 1024.0 * 1024 * 1024;
  return v > 0 ? (uint64_t)(v * mul) : 0;
}

static int init_common(nt_ctx** out, const std::vector<int>& ords) {
  if (!out) return NT_EINVAL;
  *out = nullptr;
  auto ctx = std::make_unique<nt_ctx>();
  ctx->small_model = small_model_with_env(NtSmallModel{});
  ctx->hbm_budget = env_budget();
  const int slots = std::max(1, std::min(8, (int)env_slots()));
  for (int o : ords) {
    auto d = std::make_unique<Device>();
    int rc = d->init(o, (int)ctx->devs.size());
    if (rc != NT_OK) return rc;
    d->budget->limit = ctx->hbm_budget;
    for (int k = 1; k < slots; ++k) {
      auto x = std::make_unique<Device>();
      rc = x->init(o, (int)ctx->devs.size(), d.get());
      if (rc != NT_OK) return rc;
      d->extra.push_back(std::move(x));
    }
    ctx->devs.push_back(std::move(d));
  }
  if (ctx->devs.empty()) return NT_ENODEV;
  // NT_KEY_CACHE=<max_keys>[:<admit_after>]: the key registry (nt_set_key_cache)
  if (const char* e = std::getenv("NT_KEY_CACHE")) {
    const long k = std::atol(e);
    const char* c = std::strchr(e, ':');
    const long a = c ? std::atol(c + 1) : 1;
    if (k > 0) {
      const int rc = nt_set_key_cache(ctx.get(), (uint32_t)std::min<long>(k, NT_KEY_CACHE_MAX), (uint32_t)std::max(1L, a));
      if (rc != NT_OK) return rc;
    }
  }
  *out = ctx.release();
  return NT_OK;
}

int nt_init(nt_ctx** out, int num_gpus) {
  if (num_gpus < 0) return NT_ENODEV;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return NT_ENODEV;
  if (num_gpus == 0 || num_gpus > count) num_gpus = count;
  std::vector<int> ords;
  for (int i = 0; i < num_gpus; ++i) ords.push_back(i);
  return init_common(out, ords);
}

int nt_init_device(nt_ctx** out, int device_ordinal) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return NT_ENODEV;
  if (device_ordinal < 0 || device_ordinal >= count) return NT_EINVAL;
  return init_common(out, {device_ordinal});
}

int nt_init_devices(nt_ctx** out, const int* ordinals, int n) {
  int count = 0;
  if (!ordinals || n <= 0) return NT_EINVAL;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return NT_ENODEV;
  std::vector<int> ords(ordinals, ordinals + n);
  for (int o : ords)
    if (o < 0 || o >= count) return NT_EINVAL;
  return init_common(out, ords);
}

void nt_free(nt_ctx* ctx) { delete ctx; }

int nt_num_devices(const nt_ctx* ctx) { return ctx ? (int)ctx->devs.size() : 0; }

int nt_set_hbm_budget(nt_ctx* ctx, uint64_t bytes_per_device) {
  if (!ctx) return NT_EINVAL;
  ctx->hbm_budget = bytes_per_device;
  for (auto& d : ctx->devs) {
    std::lock_guard<std::mutex> lk(d->budget->mu);
    d->budget->limit = bytes_per_device;
  }
  return NT_OK;
}

// nt_memory_info(ctx, dev | NT_INFO_KTAB, out8): the key-table cache of device entry `dev`
static int ktab_info(nt_ctx* ctx, int dev, uint64_t* out8) {
  if (!ctx || !out8 || dev < 0 || dev >= (int)ctx->devs.size()) return NT_EINVAL;
  Device& e = *ctx->devs[dev];
  uint64_t v[8] = {};
  void* slots = nullptr;
  {
    std::lock_guard<std::mutex> lk(e.tables_mu);
    slots = e.d_kslots;
    v[1] = e.kcap;
    v[2] = e.ktab_reserved;
    v[6] = slots ? nt::kKTabIndexSlots : 0;
  }
  if (slots) {
    uint32_t ctl[nt::kKTabCtlWords] = {};
    if (hipSetDevice(e.ordinal) != hipSuccess ||
        hipMemcpy(ctl, slots, sizeof ctl, hipMemcpyDeviceToHost) != hipSuccess)
      return NT_EHIP;
    v[0] = std::min<uint64_t>(ctl[0], v[1]);  // the bump counter may run past a full pool
    v[3] = ctl[1];
    v[4] = ctl[2];
    v[5] = ctl[3];
  }
  std::memcpy(out8, v, sizeof v);
  return NT_OK;
}

int nt_memory_info(nt_ctx* ctx, int dev, uint64_t* out8) {
  if (dev >= 0 && (dev & NT_INFO_KTAB)) return ktab_info(ctx, dev & ~NT_INFO_KTAB, out8);
  if (!ctx || !out8 || dev < 0 || dev >= (int)ctx->devs.size()) return NT_EINVAL;
  Device& e = *ctx->devs[dev];
  uint64_t ws = 0, stash = 0, staging = 0;
  std::vector<Device*> slots{&e};
  for (auto& x : e.extra) slots.push_back(x.get());
  for (Device* sl : slots) {
    std::lock_guard<std::mutex> lk(sl->mu);
    // ws: both lanes' workspaces; stash: both lanes' stash + sort scratch; staging: all of d[]
    for (const Lane& l : sl->lane) {
      ws += l.ws.cap;
      stash += l.stash.cap + l.sort.cap;
    }
    for (const DevBuf& b : sl->d) staging += b.cap;
  }
  uint64_t comb_bits = 0, comb_bytes = 0, reserved = 0;
  {
    std::lock_guard<std::mutex> lk(e.tables_mu);
    if (e.combB) {
      comb_bits = (uint64_t)e.bbits;
      comb_bytes = nt::wcomb_bytes_per_key(e.bbits);
    }
    reserved = e.comb_reserved;
  }
  uint64_t limit = 0, held = 0;
  {
    std::lock_guard<std::mutex> lk(e.budget->mu);
    limit = e.budget->limit;
    held = e.budget->held;
  }
  const uint64_t v[8] = {comb_bits, comb_bytes, held - std::min(held, reserved), ws, stash, staging, limit, held};
  std::memcpy(out8, v, sizeof v);
  return NT_OK;
}

int nt_set_small_call_path(nt_ctx* ctx, int mode, int threads) {
  if (!ctx || mode < NT_SMALL_OFF || mode > NT_SMALL_ALWAYS) return NT_EINVAL;
  if (threads <= 0) threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  threads = std::min(threads, nt::cpu::pool_threads());  // the host lane's real parallelism
  ctx->small_mode = NT_SMALL_OFF;  // calibration runs the GPU paths
  ctx->small_threads = threads;
  if (mode != NT_SMALL_OFF) {
    nt::cpu::init(threads);
    if (!ctx->small_model.calibrated) {
      const int rc = calibrate_small(ctx);
      if (rc != NT_OK) return rc;
    }
  }
  ctx->small_mode = mode;
  return NT_OK;
}

int nt_small_call_model(const nt_ctx* ctx, double* out10) {
  if (!ctx || !out10) return NT_EINVAL;
  const NtSmallModel& m = ctx->small_model;
  const double v[10] = {m.cpu_verify_us, m.gpu_verify_us, m.cpu_sha_mbs, m.gpu_lane_mbs, m.gpu_call_us,
                        m.pcie_gbs,      m.spawn_us,      (double)ctx->small_threads.load(), (double)m.calibrated,
                        m.gpu_keyset_us};
  std::memcpy(out10, v, sizeof v);
  return NT_OK;
}

int nt_call_counts(const nt_ctx* ctx, uint64_t* host_calls, uint64_t* gpu_calls) {
  if (!ctx) return NT_EINVAL;
  if (host_calls) *host_calls = ctx->calls_host.load();
  if (gpu_calls) *gpu_calls = ctx->calls_gpu.load();
  return NT_OK;
}

void* nt_host_alloc(uint64_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, std::max<uint64_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_pin_mu);
  g_pinned[(uintptr_t)p] = std::max<uint64_t>(bytes, 1);
  return p;
}

void nt_host_free(void* p) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pinned.erase((uintptr_t)p);
  }
  (void)hipHostFree(p);
}

}  // extern "C"
