// nt_device_probe.hip -- TEST INFRASTRUCTURE: the device runner of the arithmetic probe: the
// device functions of narwhal-tusk_amd/csrc/*.hpp compiled for gfx950 with the product's
// flags, so that the arithmetic tests can hand the GPU build the inputs a signature never
// steers to it (tests/test_gpu_device_arith.py).
// The per-item entry points (ntp_*) are those of nt_probe_entries.inc, shared with the host
// harness; this file is what they run on: one kernel template, k_item, around the items of
// nt_probe_items.hpp, and run(), which gives every described argument a device allocation.
// Thread i of the grid runs item i, so with blocks of kBlock = 256 item i sits in wave i / 64,
// lane i % 64, and a test chooses what shares a wave.  Each ntp_* entry point takes host
// pointers, works on device 0 with one launch and returns the hipError_t (0 = success).
// Written here by hand is what has no host twin of the same shape: the wide combs, over a
// comb set that ntp_wcomb_build makes with the product's own k_wcomb_bases / k_wcomb_fill
// through wcomb_build<W> (csrc/wcomb_build.hpp) and that stays live on the device (entries,
// sums, key sums; its key 0 is ntp_verify_kc's comb of B), and ntp_key_sort, the product's
// counting sort (csrc/key_sort.hpp launch_key_sort: k_key_hist, k_key_scatter) handing back
// the permutation a key-cache launch would walk.
// Never linked into libntcrypto.so.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <tuple>

#include "../../narwhal-tusk_amd/csrc/kernels_common.hpp"
#include "../../narwhal-tusk_amd/csrc/key_sort.hpp"
#include "nt_probe_items.hpp"

using namespace nt;
using namespace ntp;

namespace {

// A device buffer of `bytes` bytes, filled from `host` (when given); the first
// error of a chain of buffers and copies is kept in *err.
struct Dev {
  void* p = nullptr;
  hipError_t* err = nullptr;
  Dev() = default;
  Dev(hipError_t* e, const void* host, size_t bytes) { put(e, host, bytes); }
  void put(hipError_t* e, const void* host, size_t bytes) {
    err = e;
    if (*err != hipSuccess) return;
    *err = hipMalloc(&p, bytes ? bytes : 1);
    if (*err == hipSuccess && host && bytes) *err = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
  }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  ~Dev() {
    if (p) (void)hipFree(p);
  }
  void back(void* host, size_t bytes) const {
    if (*err == hipSuccess && bytes) *err = hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost);
  }
  template <class T>
  T* as() const { return (T*)p; }
};

inline unsigned grid(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
__device__ inline uint64_t item_index() { return (uint64_t)blockIdx.x * kBlock + threadIdx.x; }

// after the launch: launch error, then the kernel's own
inline void finish(hipError_t* err) {
  if (*err != hipSuccess) return;
  *err = hipGetLastError();
  if (*err == hipSuccess) *err = hipDeviceSynchronize();
}

// ---- run(): what the entries of nt_probe_entries.inc run on.  up() gives a described argument
// its device allocation (d) and returns the kernel's argument, down() copies results back.
template <class T>
const T* up(hipError_t* e, Dev& d, uint64_t n, In<T> a) {
  d.put(e, a.p, a.bytes * n);
  return d.as<const T>();
}
template <class T>
T* up(hipError_t* e, Dev& d, uint64_t n, Out<T> a) {
  d.put(e, nullptr, a.bytes * n);
  return d.as<T>();
}
struct WsArg {  // every block's slice of the workspace; the kernel makes the lane's WsATab of it
  uint4* ws;
};
WsArg up(hipError_t* e, Dev& d, uint64_t n, Ws) {
  d.put(e, nullptr, (size_t)grid(n) * kBlock * kAEntries * kAQuads * sizeof(uint4));
  return WsArg{d.as<uint4>()};
}
// The product's DevKTab over a copy of the caller's blob: words 4..6 of the control block -- the
// pool's address and slots - 1 -- and, with a comb pool, words 8..9 -- its address, behind the
// entries -- are written from the host before the launch and zeroed again on the way back.
static_assert(DevKTab::kComb, "the probe is built with the product's defaults: the second pool holds combs");
template <bool COMB>
DevKTab up(hipError_t* e, Dev& d, uint64_t, Blob<COMB> b) {
  d.put(e, b.p, b.bytes());
  const unsigned long long pool = (uintptr_t)d.p + kKtProbePoolOff, comb = (uintptr_t)d.p + kcomb_probe_comb_off(b.cap);
  const uint32_t w[3] = {(uint32_t)pool, (uint32_t)(pool >> 32), kKtProbeSlots - 1u};
  const uint32_t c[2] = {(uint32_t)comb, (uint32_t)(comb >> 32)};
  if (*e == hipSuccess) *e = hipMemcpy(d.as<uint8_t>() + 16, w, sizeof w, hipMemcpyHostToDevice);
  if (COMB && *e == hipSuccess) *e = hipMemcpy(d.as<uint8_t>() + 32, c, sizeof c, hipMemcpyHostToDevice);
  return DevKTab{d.as<uint32_t>(), b.cap};
}
DevKTab up(hipError_t*, Dev&, uint64_t, NoTable) { return DevKTab{nullptr, 0}; }  // the LDS digit cells alone
// a 256-byte aligned allocation; load_words reads whole 4-byte granules: a multiple of 16 past the end
const uint8_t* up(hipError_t* e, Dev& d, uint64_t, Msg m) {
  const size_t padded = (size_t)((m.bytes + 15) / 16 * 16 + 16);
  d.put(e, nullptr, padded);
  if (*e == hipSuccess) *e = hipMemset(d.p, 0, padded);
  if (*e == hipSuccess && m.bytes) *e = hipMemcpy(d.p, m.p, m.bytes, hipMemcpyHostToDevice);
  return d.as<const uint8_t>();
}
template <class V>
V up(hipError_t*, Dev&, uint64_t, V v) { return v; }  // a Const, the comb of B: as it is

template <class T>
void down(const Dev& d, uint64_t n, Out<T> a) { d.back(a.p, a.bytes * n); }
template <bool COMB>
void down(const Dev& d, uint64_t, Blob<COMB> b) {
  d.back(b.p, b.bytes());
  if (*d.err != hipSuccess) return;
  std::memset(b.p + 16, 0, 12);
  if (COMB) std::memset(b.p + 32, 0, 8);
}
template <class V>
void down(const Dev&, uint64_t, V) {}

template <class K>
__device__ inline K lane(K k) { return k; }
__device__ inline WsATab lane(WsArg w) { return WsATab{w.ws, blockIdx.x}; }

// The one kernel of the entries: thread i runs item i.  Tail says what the lanes past n do
// (nt_probe_items.hpp Leave, Repeat); which of the two an entry takes decides what its
// wave-level operations (fe_invert_vt's exit, wave_max, the wave-uniform builds) see.
template <class Tail, class Item, class... K>
__global__ void __launch_bounds__(kBlock) k_item(uint64_t n, Item item, K... k) {
  const uint64_t i = item_index();
  if constexpr (std::is_same<Tail, Repeat>::value) item(i < n ? i : n - 1, lane(k)..., i < n);
  else if (i < n) item(i, lane(k)...);
}

// inputs in (left to right: the first error of the chain is the one returned, and nothing is
// launched after one), one launch of grid(n) blocks, outputs and blob back
template <class Tail, class Item, class... A>
int run(uint64_t n, Item item, A... a) {
  hipError_t err = hipSetDevice(0);
  if (n == 0) return (int)err;
  Dev d[sizeof...(A)], *q = d;
  const std::tuple k{up(&err, *q++, n, a)...};
  std::apply([&](auto... ka) {
    if (err == hipSuccess) k_item<Tail><<<dim3(grid(n)), dim3(kBlock), 0, 0>>>(n, item, ka...);
  }, k);
  finish(&err);
  q = d;
  (down(*q++, n, a), ...);
  return (int)err;
}

// The wide-comb kernels: the product's WideComb<W> over the probe's comb set (key[i] picks
// the comb of item i).  Lanes past n leave at once: key_comb_sum's wave_any then sees
// exactly the lanes the caller filled.
template <int W>
__global__ void __launch_bounds__(kBlock) k_wcomb_entries(uint64_t n, const uint32_t* comb, const uint32_t* key,
                                                          const uint32_t* pos, const uint32_t* idx, uint32_t* o) {
  const uint64_t i = item_index();
  if (i >= n) return;
  const WideComb<W> wc{comb + (size_t)key[i] * CombGeom<W>::kWordsPerPoint};
  ntp::item_wcomb_entry(i, wc, pos[i], idx[i], o);
}
template <int W>
__global__ void __launch_bounds__(kBlock)
    k_wcomb_acc(uint64_t n, const uint32_t* comb, const uint32_t* key, const uint32_t* x, const uint32_t* flags,
                const uint32_t* start, uint32_t* o) {
  const uint64_t i = item_index();
  if (i >= n) return;
  const WideComb<W> wc{comb + (size_t)key[i] * CombGeom<W>::kWordsPerPoint};
  ntp::item_wcomb_acc(i, wc, x, flags, start, o);
}
template <int W>
__global__ void __launch_bounds__(kBlock) k_key_comb_sum(uint64_t n, const uint32_t* comb, const uint32_t* key,
                                                         const uint32_t* meta, const uint32_t* k, uint32_t* o) {
  const uint64_t i = item_index();
  if (i >= n) return;
  const WideComb<W> wc{comb + (size_t)key[i] * CombGeom<W>::kWordsPerPoint};
  ntp::item_key_comb_sum(i, wc, meta, k, o);
}

// The probe's comb set: `nkeys` combs of `bits`-bit digits in one allocation, then
// ntp::kWcGuardBytes of the fill pattern.  One set is live at a time.
struct WcSet {
  int bits = 0;
  uint32_t nkeys = 0;
  uint8_t* p = nullptr;
  size_t comb_bytes = 0;
} g_wc;

void wc_free() {
  if (g_wc.p) (void)hipFree(g_wc.p);
  g_wc = WcSet{};
}
// the `guard` bytes at d still hold the fill pattern
bool guard_intact(hipError_t* err, const uint8_t* d, size_t guard) {
  static uint8_t h[ntp::kWcGuardBytes];
  if (*err == hipSuccess) *err = hipMemcpy(h, d, guard, hipMemcpyDeviceToHost);
  if (*err != hipSuccess) return false;
  for (size_t b = 0; b < guard; ++b)
    if (h[b] != (uint8_t)ntp::kWcFill) return false;
  return true;
}

// key 0 of the live comb set as verify_kc's comb of B: the narrowest width
inline bool live_bcomb_ok() { return g_wc.p && g_wc.bits == kKeyCombNarrow; }
inline WideComb<kKeyCombNarrow> live_bcomb() { return WideComb<kKeyCombNarrow>{(const uint32_t*)g_wc.p}; }

}  // namespace

#define NTP_NAME(name) ntp_##name
#include "nt_probe_entries.inc"

#define NTP_BEGIN                     \
  hipError_t err = hipSetDevice(0);    \
  if (n == 0) return (int)err;
#define NTP_LAUNCH(kernel, ...) \
  if (err == hipSuccess) hipLaunchKernelGGL(kernel, dim3(grid(n)), dim3(kBlock), 0, 0, n, __VA_ARGS__); \
  finish(&err);

extern "C" {

// ---- the wide combs.  Every index a kernel below forms is checked here, on the host, against
// the live comb set before anything is launched (ntp::*_args_ok): nothing out of range reaches
// the GPU.
// Builds the combs of nkeys encodings (negate: of the negated points) with the product's
// wcomb_build<W>, `batch` keys per fill launch and the scratch sizes the product allocates for
// that batch, into an allocation pre-filled with 0xA5 that stays alive until ntp_wcomb_free or
// the next build; meta_out = the kKey* words.  The builders' scratch (bases, tmp) is followed by
// the same guard pattern: hipErrorUnknown if a build wrote past either.
int ntp_wcomb_build(int bits, uint32_t nkeys, const uint32_t* enc8, int negate, uint32_t batch, uint32_t* meta_out) {
  if (!ntp::wcomb_build_args_ok(bits, nkeys, negate, batch)) return (int)hipErrorInvalidValue;
  hipError_t err = hipSetDevice(0);
  wc_free();
  const size_t comb_bytes = comb_size(bits, 0) * nkeys, bases_bytes = comb_size(bits, 1) * nkeys,
               tmp_bytes = comb_size(bits, 2) * (batch < nkeys ? batch : nkeys), guard = ntp::kWcGuardBytes;
  if (err == hipSuccess) err = hipMalloc((void**)&g_wc.p, comb_bytes + guard);
  if (err != hipSuccess) {
    g_wc = WcSet{};
    return (int)err;
  }
  g_wc.bits = bits;
  g_wc.nkeys = nkeys;
  g_wc.comb_bytes = comb_bytes;
  err = hipMemset(g_wc.p, ntp::kWcFill, comb_bytes + guard);
  Dev de(&err, enc8, 32 * (size_t)nkeys), dm(&err, nullptr, 4 * (size_t)nkeys), db(&err, nullptr, bases_bytes + guard),
      dt(&err, nullptr, tmp_bytes + guard);
  if (err == hipSuccess) err = hipMemset((uint8_t*)db.p + bases_bytes, ntp::kWcFill, guard);
  if (err == hipSuccess) err = hipMemset((uint8_t*)dt.p + tmp_bytes, ntp::kWcFill, guard);
  if (err == hipSuccess)
    ntp::wcomb_width(bits, [&](auto w) {
      err = wcomb_build<decltype(w)::value>(de.as<uint32_t>(), nkeys, negate, (uint32_t*)g_wc.p, dm.as<uint32_t>(),
                                            db.as<uint32_t>(), dt.as<uint32_t>(), batch, 0);
    });
  if (err == hipSuccess) err = hipDeviceSynchronize();
  dm.back(meta_out, 4 * (size_t)nkeys);
  const bool scratch_ok = guard_intact(&err, (uint8_t*)db.p + bases_bytes, guard) &&
                          guard_intact(&err, (uint8_t*)dt.p + tmp_bytes, guard);
  if (err == hipSuccess && !scratch_ok) err = hipErrorUnknown;
  if (err != hipSuccess) wc_free();
  return (int)err;
}
int ntp_wcomb_free() {
  wc_free();
  return 0;
}
// out1 = 1: the guard after the live comb set still holds the fill pattern
int ntp_wcomb_guard(uint32_t* out1) {
  if (!g_wc.p) return (int)hipErrorInvalidValue;
  hipError_t err = hipSetDevice(0);
  *out1 = guard_intact(&err, g_wc.p + g_wc.comb_bytes, ntp::kWcGuardBytes) ? 1u : 0u;
  return (int)err;
}
// needs no table (the loads go to a recording comb): any 256-bit x
int ntp_wcomb_entries(uint64_t n, const uint32_t* key, const uint32_t* pos, const uint32_t* idx, uint32_t* out32) {
  bool ok = false;
  ntp::wcomb_width(g_wc.bits, [&](auto w) { ok = ntp::wcomb_entry_args_ok<decltype(w)::value>(n, g_wc.nkeys, key, pos, idx); });
  if (!g_wc.p || !ok) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  Dev dk(&err, key, 4 * n), dp(&err, pos, 4 * n), di(&err, idx, 4 * n), dout(&err, nullptr, 128 * n);
  ntp::wcomb_width(g_wc.bits, [&](auto w) {
    NTP_LAUNCH(k_wcomb_entries<decltype(w)::value>, (const uint32_t*)g_wc.p, dk.as<uint32_t>(), dp.as<uint32_t>(),
               di.as<uint32_t>(), dout.as<uint32_t>())
  });
  dout.back(out32, 128 * n);
  return (int)err;
}
int ntp_wcomb_acc(uint64_t n, const uint32_t* key, const uint32_t* x8, const uint32_t* flags, const uint32_t* start_enc8,
                  uint32_t* out_enc8) {
  bool ok = false;
  ntp::wcomb_width(g_wc.bits, [&](auto w) { ok = ntp::wcomb_acc_args_ok<decltype(w)::value>(n, g_wc.nkeys, key, x8, flags); });
  if (!g_wc.p || !ok) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  Dev dk(&err, key, 4 * n), dx(&err, x8, 32 * n), df(&err, flags, 4 * n), ds(&err, start_enc8, 32 * n),
      dout(&err, nullptr, 32 * n);
  ntp::wcomb_width(g_wc.bits, [&](auto w) {
    NTP_LAUNCH(k_wcomb_acc<decltype(w)::value>, (const uint32_t*)g_wc.p, dk.as<uint32_t>(), dx.as<uint32_t>(),
               df.as<uint32_t>(), ds.as<uint32_t>(), dout.as<uint32_t>())
  });
  dout.back(out_enc8, 32 * n);
  return (int)err;
}
int ntp_key_comb_sum(uint64_t n, const uint32_t* key, const uint32_t* meta, const uint32_t* k8, uint32_t* out_enc8) {
  bool ok = false;
  ntp::wcomb_width(g_wc.bits, [&](auto w) { ok = ntp::key_comb_args_ok<decltype(w)::value>(n, g_wc.nkeys, key, k8); });
  if (!g_wc.p || !ok) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  Dev dk(&err, key, 4 * n), dm(&err, meta, 4 * n), ds(&err, k8, 32 * n), dout(&err, nullptr, 32 * n);
  ntp::wcomb_width(g_wc.bits, [&](auto w) {
    NTP_LAUNCH(k_key_comb_sum<decltype(w)::value>, (const uint32_t*)g_wc.p, dk.as<uint32_t>(), dm.as<uint32_t>(),
               ds.as<uint32_t>(), dout.as<uint32_t>())
  });
  dout.back(out_enc8, 32 * n);
  return (int)err;
}


// perm_out[0 .. n) = the key-grouped order of key[0 .. n) (slot -> signature), as
// launch_verify_keyset gets it: bucket lines zeroed, then launch_key_sort.  Device-only
// (no host twin: the sort is two kernels, not a device function of the headers).
int ntp_key_sort(uint64_t n, const uint32_t* key, int mixed, uint32_t nkeys, uint32_t* perm_out) {
  NTP_BEGIN
  if (nkeys + 1 > kSortBuckets || n > 0xFFFFFFFFull) return (int)hipErrorInvalidValue;
  const size_t line_bytes = 4ull * kCtrStride * (nkeys + 1);
  Dev dkey(&err, key, 4 * n), dlines(&err, nullptr, line_bytes), dperm(&err, nullptr, 4 * n);
  if (err == hipSuccess) err = hipMemset(dlines.p, 0, line_bytes);
  if (err == hipSuccess) err = hipMemset(dperm.p, 0xFF, 4 * n);
  if (err == hipSuccess) err = launch_key_sort(dkey.as<uint32_t>(), n, mixed, nkeys, dlines.as<uint32_t>(),
                                              dperm.as<uint32_t>(), 0);
  finish(&err);
  dperm.back(perm_out, 4 * n);
  return (int)err;
}


}  // extern "C"
