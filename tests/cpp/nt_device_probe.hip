// nt_device_probe.hip -- TEST INFRASTRUCTURE: the device functions of
// narwhal-tusk_amd/csrc/*.hpp behind one kernel each, compiled for gfx950 with
// the product's flags, so that the arithmetic tests can hand the GPU build the
// inputs a signature never steers to it (tests/test_gpu_device_arith.py).
// Every kernel is a thin wrapper around nt_probe_items.hpp (the same item
// functions the host harness loops over): thread i of the grid runs item i, so
// with blocks of kBlock = 256 item i sits in wave i / 64, lane i % 64, and a
// test chooses what shares a wave.  Each ntp_* entry point takes host pointers,
// works on device 0 and returns the hipError_t (0 = success).
// Kernels: k_fe_* (multiply, squares, carry, bytes, both inversions), k_sc_* (reduce512,
// muladd, mul, reduce_half, recode_w4, is_canonical, halfsize, unbalanced), k_hram,
// k_point_checks, k_ladder_uv, the key-table cache's k_ktab_fill / k_ktab_point /
// k_ladder_uv3, and the wide combs': k_wcomb_digits (wcomb_digit under wcomb_acc's
// schedule), k_wcomb_entries (WideComb::load / load_corr), k_wcomb_acc, k_key_comb_sum --
// the last three over combs that ntp_wcomb_build makes with the product's own
// k_wcomb_bases / k_wcomb_fill through wcomb_build<W> (csrc/wcomb_build.hpp).
// The comb path of the key-table cache runs over a second blob (nt_probe_items.hpp
// kcomb_probe_bytes: the key table, then a comb pool whose address words 8..9 of the control block
// carry, then a guard), so DevKTab::has_comb() holds as in the product: k_kcomb_fill (probe, take,
// ktab_build_comb with the lane's WsATab), k_kcomb_line (DevKTab::comb_load and comb_line's clamp),
// k_kc_picks (kc_recode / kc_pick through the LDS digit cells), k_ladder_kc, k_compare_one and
// k_verify_kc, the last with the narrowest comb of B that ntp_wcomb_build makes.  The three-table
// kernels keep their blob, in which words 8..9 stay zero.
// ntp_key_sort runs the product's counting sort (csrc/key_sort.hpp launch_key_sort: k_key_hist,
// k_key_scatter) and hands back the permutation a key-cache launch would walk.
// Never linked into libntcrypto.so.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../narwhal-tusk_amd/csrc/kernels_common.hpp"
#include "../../narwhal-tusk_amd/csrc/key_sort.hpp"
#include "nt_probe_items.hpp"

using namespace nt;

namespace {

// A device buffer of `bytes` bytes, filled from `host` (when given); the first
// error of a chain of buffers and copies is kept in *err.
struct Dev {
  void* p = nullptr;
  hipError_t* err;
  Dev(hipError_t* e, const void* host, size_t bytes) : err(e) {
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

__global__ void __launch_bounds__(kBlock) k_fe_mul(uint64_t n, const uint32_t* f, const uint32_t* g, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_fe_mul(i, f, g, o);
}
// which: 0 fe_sq, 1 fe_sq_wide, 2 fe_carry
__global__ void __launch_bounds__(kBlock) k_fe_unary(uint64_t n, const uint32_t* f, uint32_t* o, int which) {
  const uint64_t i = item_index();
  if (i >= n) return;
  if (which == 0) ntp::item_fe_sq(i, f, o);
  else if (which == 1) ntp::item_fe_sq_wide(i, f, o);
  else ntp::item_fe_carry(i, f, o);
}
__global__ void __launch_bounds__(kBlock) k_fe_tobytes(uint64_t n, const uint32_t* f, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_fe_tobytes(i, f, o);
}
__global__ void __launch_bounds__(kBlock) k_fe_frombytes(uint64_t n, const uint32_t* in, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_fe_frombytes(i, in, o);
}
// Lanes past n leave at once, so the wave-level exit of fe_invert_vt sees
// exactly the lanes the caller filled.
__global__ void __launch_bounds__(kBlock) k_fe_invert_vt(uint64_t n, const uint32_t* f, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_fe_invert(i, f, o, 1);
}
__global__ void __launch_bounds__(kBlock) k_fe_invert(uint64_t n, const uint32_t* f, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_fe_invert(i, f, o, 0);
}
__global__ void __launch_bounds__(kBlock) k_sc_reduce512(uint64_t n, const uint32_t* in, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_sc_reduce512(i, in, o);
}
__global__ void __launch_bounds__(kBlock)
    k_sc_muladd(uint64_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_sc_muladd(i, a, b, c, o);
}
__global__ void __launch_bounds__(kBlock) k_sc_mul(uint64_t n, const uint32_t* a, const uint32_t* b, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_sc_mul(i, a, b, o);
}
__global__ void __launch_bounds__(kBlock) k_sc_reduce_half(uint64_t n, const uint32_t* k, uint32_t* o, uint32_t* neg) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_sc_reduce_half(i, k, o, neg);
}
__global__ void __launch_bounds__(kBlock) k_sc_recode_w4(uint64_t n, const uint32_t* s, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_sc_recode_w4(i, s, o);
}
__global__ void __launch_bounds__(kBlock) k_sc_is_canonical(uint64_t n, const uint32_t* s, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_sc_is_canonical(i, s, o);
}
template <bool LEHMER>
__global__ void __launch_bounds__(kBlock)
    k_sc_halfsize(uint64_t n, const uint32_t* k, uint32_t* u, uint32_t* uneg, uint32_t* v, int32_t* bits) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_sc_halfsize(i, k, u, uneg, v, bits, LEHMER ? 1 : 0);
}
template <bool FAST>
__global__ void __launch_bounds__(kBlock) k_hram(uint64_t n, const uint32_t* R, const uint32_t* A, const uint8_t* msg,
                                                 const uint64_t* off, const uint64_t* len, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_hram(i, R, A, msg, off, len, o, FAST ? 1 : 0);
}
__global__ void __launch_bounds__(kBlock) k_point_checks(uint64_t n, const uint32_t* enc, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_point_checks(i, enc, o);
}
// Lanes past n run the last item again (and write nothing): wave_max shuffles
// across all 64 lanes of a wave, so every lane of a launched wave stays active.
__global__ void __launch_bounds__(kBlock)
    k_ladder_uv(uint64_t n, const uint32_t* A, const uint32_t* R, const uint32_t* u, const uint32_t* uneg,
                const uint32_t* v, const int32_t* bits, uint4* ws, uint32_t* o) {
  const uint64_t i = item_index();
  WsATab at{ws, blockIdx.x};
  ntp::item_ladder_uv(i < n ? i : n - 1, A, R, u, uneg, v, bits, at, o, i < n);
}

template <bool LEHMER>
__global__ void __launch_bounds__(kBlock) k_sc_unbalanced(uint64_t n, const uint32_t* k, uint32_t* u, uint32_t* uneg,
                                                          uint32_t* v, int32_t* ubits, int32_t* vbits) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_sc_unbalanced(i, k, u, uneg, v, ubits, vbits, LEHMER ? 1 : 0);
}
// The key-table cache kernels: the product's DevKTab over the probe's allocation.
// ktab_build is wave-uniform, as in verify_n: lanes past n run it on the last key
// with no claim (they neither probe nor store).
__global__ void __launch_bounds__(kBlock)
    k_ktab_fill(uint64_t n, const uint32_t* A, uint32_t* base, uint32_t cap, uint32_t* slot) {
  const uint64_t i = item_index();
  const DevKTab kt{base, cap};
  ntp::item_ktab_fill(i < n ? i : n - 1, A, kt, slot, i < n);
}
__global__ void __launch_bounds__(kBlock) k_ktab_point(uint64_t n, const uint32_t* A, const int32_t* td, uint32_t* base,
                                                       uint32_t cap, uint32_t* out3, uint32_t* enc) {
  const uint64_t i = item_index();
  const DevKTab kt{base, cap};
  if (i < n) ntp::item_ktab_point(i, A, td, kt, out3, enc);
}
// lanes past n run the last item again and write nothing (wave_max: see k_ladder_uv)
__global__ void __launch_bounds__(kBlock)
    k_ladder_uv3(uint64_t n, const uint32_t* kidx, const uint32_t* R, const uint32_t* u, const uint32_t* v,
                 const uint32_t* sc4, uint32_t* base, uint32_t cap, uint4* ws, uint32_t* o) {
  const uint64_t i = item_index();
  WsATab at{ws, blockIdx.x};
  const DevKTab kt{base, cap};
  ntp::item_ladder_uv3(i < n ? i : n - 1, kidx, R, u, v, sc4, at, kt, o, i < n);
}

// The probe's key table on the device: `blob` (ktab_probe_bytes(cap) bytes, owned by the
// caller) copied in, words 4..6 of the control block -- the pool's address and slots - 1 --
// written from the host before the launch, and copied back after it with those three zeroed.
// comb: the blob of the comb items (kcomb_probe_bytes(cap) bytes), words 8..9 carrying the
// address of the comb pool behind the entries, zeroed again on the way back.
struct DevBlob {
  Dev d;
  uint8_t* host;
  size_t bytes;
  bool comb;
  DevBlob(hipError_t* e, uint8_t* blob, uint32_t cap, bool with_comb = false)
      : d(e, blob, with_comb ? ntp::kcomb_probe_bytes(cap) : ntp::ktab_probe_bytes(cap)), host(blob),
        bytes(with_comb ? ntp::kcomb_probe_bytes(cap) : ntp::ktab_probe_bytes(cap)), comb(with_comb) {
    if (*e != hipSuccess) return;
    const unsigned long long pool = (unsigned long long)(uintptr_t)((uint8_t*)d.p + ntp::kKtProbePoolOff);
    const uint32_t w[3] = {(uint32_t)pool, (uint32_t)(pool >> 32), ntp::kKtProbeSlots - 1u};
    *e = hipMemcpy((uint8_t*)d.p + 16, w, sizeof w, hipMemcpyHostToDevice);
    if (*e != hipSuccess || !comb) return;
    const unsigned long long cp = (unsigned long long)(uintptr_t)((uint8_t*)d.p + ntp::kcomb_probe_comb_off(cap));
    const uint32_t c[2] = {(uint32_t)cp, (uint32_t)(cp >> 32)};
    *e = hipMemcpy((uint8_t*)d.p + 32, c, sizeof c, hipMemcpyHostToDevice);
  }
  void back() const {
    d.back(host, bytes);
    if (*d.err != hipSuccess) return;
    std::memset(host + 16, 0, 12);
    if (comb) std::memset(host + 32, 0, 8);
  }
};

// The comb kernels of the key-table cache: DevKTab over the comb blob (kComb is true under the
// product's default flags, so has_comb() holds and ktab_build takes ktab_build_comb), the
// lane's WsATab as the verify kernel hands it over.  The build is wave-uniform: lanes past n
// run it on the last key with no claim.
static_assert(DevKTab::kComb, "the probe is built with the product's defaults: the second pool holds combs");
__global__ void __launch_bounds__(kBlock)
    k_kcomb_fill(uint64_t n, const uint32_t* A, uint32_t* base, uint32_t cap, uint4* ws, uint32_t* slot) {
  const uint64_t i = item_index();
  WsATab at{ws, blockIdx.x};
  const DevKTab kt{base, cap};
  ntp::item_kcomb_fill(i < n ? i : n - 1, A, kt, at, slot, i < n);
}
__global__ void __launch_bounds__(kBlock) k_kcomb_line(uint64_t n, const uint32_t* A, const uint32_t* line, uint32_t* base,
                                                       uint32_t cap, uint32_t* out3, uint32_t* limbs) {
  const uint64_t i = item_index();
  const DevKTab kt{base, cap};
  if (i < n) ntp::item_kcomb_line(i, A, line, kt, out3, limbs);
}
// only the LDS digit cells of the policy are used: no table behind it
__global__ void __launch_bounds__(kBlock) k_kc_picks(uint64_t n, const uint32_t* k, uint32_t* o) {
  const uint64_t i = item_index();
  const DevKTab kt{nullptr, 0};
  if (i < n) ntp::item_kc_picks(i, k, kt, o);
}
// lanes past n run the last item again and write nothing
__global__ void __launch_bounds__(kBlock) k_ladder_kc(uint64_t n, const uint32_t* kidx, const uint32_t* k,
                                                      const uint32_t* dead, uint32_t* base, uint32_t cap, uint32_t* o) {
  const uint64_t i = item_index();
  const DevKTab kt{base, cap};
  ntp::item_ladder_kc(i < n ? i : n - 1, kidx, k, dead, kt, o, i < n);
}
// lanes past n leave at once (fe_invert_vt's wave-level exit sees the lanes the caller filled)
__global__ void __launch_bounds__(kBlock) k_compare_one(uint64_t n, const uint32_t* x, const uint32_t* y, const uint32_t* z,
                                                        const uint32_t* R, const uint32_t* mode, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_compare_one(i, x, y, z, R, mode, o);
}
// comb: the comb of B (key 0 of the live comb set); lanes past n run the last item again and write nothing
template <int W>
__global__ void __launch_bounds__(kBlock)
    k_verify_kc(uint64_t n, const uint32_t* comb, const uint32_t* kidx, const uint32_t* kflags, const uint32_t* R,
                const uint32_t* S, const uint32_t* k, const uint32_t* mode, uint32_t* base, uint32_t cap, uint32_t* o) {
  const uint64_t i = item_index();
  const DevKTab kt{base, cap};
  const WideComb<W> wb{comb};
  ntp::item_verify_kc(i < n ? i : n - 1, kidx, kflags, R, S, k, mode, wb, kt, o, i < n);
}

// The wide-comb kernels: the product's WideComb<W> over the probe's comb set (key[i] picks
// the comb of item i).  Lanes past n leave at once: key_comb_sum's wave_any then sees
// exactly the lanes the caller filled.
template <int W>
__global__ void __launch_bounds__(kBlock) k_wcomb_digits(uint64_t n, const uint32_t* x, uint32_t* o) {
  const uint64_t i = item_index();
  if (i < n) ntp::item_wcomb_digits<W>(i, x, o);
}
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

}  // namespace

#define NTP_BEGIN                     \
  hipError_t err = hipSetDevice(0);    \
  if (n == 0) return (int)err;
#define NTP_LAUNCH(kernel, ...) \
  if (err == hipSuccess) hipLaunchKernelGGL(kernel, dim3(grid(n)), dim3(kBlock), 0, 0, n, __VA_ARGS__); \
  finish(&err);

extern "C" {

int ntp_fe_mul(uint64_t n, const uint32_t* f, const uint32_t* g, uint32_t* out) {
  NTP_BEGIN
  Dev df(&err, f, 40 * n), dg(&err, g, 40 * n), dout(&err, nullptr, 40 * n);
  NTP_LAUNCH(k_fe_mul, df.as<uint32_t>(), dg.as<uint32_t>(), dout.as<uint32_t>())
  dout.back(out, 40 * n);
  return (int)err;
}
static int fe_unary(uint64_t n, const uint32_t* f, uint32_t* out, int which) {
  NTP_BEGIN
  Dev df(&err, f, 40 * n), dout(&err, nullptr, 40 * n);
  NTP_LAUNCH(k_fe_unary, df.as<uint32_t>(), dout.as<uint32_t>(), which)
  dout.back(out, 40 * n);
  return (int)err;
}
int ntp_fe_sq(uint64_t n, const uint32_t* f, uint32_t* out) { return fe_unary(n, f, out, 0); }
int ntp_fe_sq_wide(uint64_t n, const uint32_t* f, uint32_t* out) { return fe_unary(n, f, out, 1); }
int ntp_fe_carry(uint64_t n, const uint32_t* f, uint32_t* out) { return fe_unary(n, f, out, 2); }
int ntp_fe_tobytes(uint64_t n, const uint32_t* f, uint32_t* out8) {
  NTP_BEGIN
  Dev df(&err, f, 40 * n), dout(&err, nullptr, 32 * n);
  NTP_LAUNCH(k_fe_tobytes, df.as<uint32_t>(), dout.as<uint32_t>())
  dout.back(out8, 32 * n);
  return (int)err;
}
int ntp_fe_frombytes(uint64_t n, const uint32_t* in8, uint32_t* out) {
  NTP_BEGIN
  Dev din(&err, in8, 32 * n), dout(&err, nullptr, 40 * n);
  NTP_LAUNCH(k_fe_frombytes, din.as<uint32_t>(), dout.as<uint32_t>())
  dout.back(out, 40 * n);
  return (int)err;
}
int ntp_fe_invert(uint64_t n, const uint32_t* f, uint32_t* out8, int vt) {
  NTP_BEGIN
  Dev df(&err, f, 40 * n), dout(&err, nullptr, 32 * n);
  if (vt) {
    NTP_LAUNCH(k_fe_invert_vt, df.as<uint32_t>(), dout.as<uint32_t>())
  } else {
    NTP_LAUNCH(k_fe_invert, df.as<uint32_t>(), dout.as<uint32_t>())
  }
  dout.back(out8, 32 * n);
  return (int)err;
}
int ntp_sc_reduce512(uint64_t n, const uint32_t* in16, uint32_t* out8) {
  NTP_BEGIN
  Dev din(&err, in16, 64 * n), dout(&err, nullptr, 32 * n);
  NTP_LAUNCH(k_sc_reduce512, din.as<uint32_t>(), dout.as<uint32_t>())
  dout.back(out8, 32 * n);
  return (int)err;
}
int ntp_sc_muladd(uint64_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out8) {
  NTP_BEGIN
  Dev da(&err, a, 32 * n), db(&err, b, 32 * n), dc(&err, c, 32 * n), dout(&err, nullptr, 32 * n);
  NTP_LAUNCH(k_sc_muladd, da.as<uint32_t>(), db.as<uint32_t>(), dc.as<uint32_t>(), dout.as<uint32_t>())
  dout.back(out8, 32 * n);
  return (int)err;
}
int ntp_sc_mul(uint64_t n, const uint32_t* a, const uint32_t* b, uint32_t* out8) {
  NTP_BEGIN
  Dev da(&err, a, 32 * n), db(&err, b, 32 * n), dout(&err, nullptr, 32 * n);
  NTP_LAUNCH(k_sc_mul, da.as<uint32_t>(), db.as<uint32_t>(), dout.as<uint32_t>())
  dout.back(out8, 32 * n);
  return (int)err;
}
int ntp_sc_reduce_half(uint64_t n, const uint32_t* k8, uint32_t* out8, uint32_t* neg) {
  NTP_BEGIN
  Dev dk(&err, k8, 32 * n), dout(&err, nullptr, 32 * n), dneg(&err, nullptr, 4 * n);
  NTP_LAUNCH(k_sc_reduce_half, dk.as<uint32_t>(), dout.as<uint32_t>(), dneg.as<uint32_t>())
  dout.back(out8, 32 * n);
  dneg.back(neg, 4 * n);
  return (int)err;
}
int ntp_sc_recode_w4(uint64_t n, const uint32_t* s8, uint32_t* out8) {
  NTP_BEGIN
  Dev ds(&err, s8, 32 * n), dout(&err, nullptr, 32 * n);
  NTP_LAUNCH(k_sc_recode_w4, ds.as<uint32_t>(), dout.as<uint32_t>())
  dout.back(out8, 32 * n);
  return (int)err;
}
int ntp_sc_is_canonical(uint64_t n, const uint32_t* s8, uint32_t* out1) {
  NTP_BEGIN
  Dev ds(&err, s8, 32 * n), dout(&err, nullptr, 4 * n);
  NTP_LAUNCH(k_sc_is_canonical, ds.as<uint32_t>(), dout.as<uint32_t>())
  dout.back(out1, 4 * n);
  return (int)err;
}
int ntp_sc_halfsize(uint64_t n, const uint32_t* k8, uint32_t* u8, uint32_t* uneg, uint32_t* v8, int32_t* bits,
                    int lehmer) {
  NTP_BEGIN
  Dev dk(&err, k8, 32 * n), du(&err, nullptr, 32 * n), dn(&err, nullptr, 4 * n), dv(&err, nullptr, 32 * n),
      db(&err, nullptr, 4 * n);
  if (lehmer) {
    NTP_LAUNCH(k_sc_halfsize<true>, dk.as<uint32_t>(), du.as<uint32_t>(), dn.as<uint32_t>(), dv.as<uint32_t>(),
               db.as<int32_t>())
  } else {
    NTP_LAUNCH(k_sc_halfsize<false>, dk.as<uint32_t>(), du.as<uint32_t>(), dn.as<uint32_t>(), dv.as<uint32_t>(),
               db.as<int32_t>())
  }
  du.back(u8, 32 * n);
  dn.back(uneg, 4 * n);
  dv.back(v8, 32 * n);
  db.back(bits, 4 * n);
  return (int)err;
}
// msg: one buffer of msg_bytes bytes (copied to a 256-byte aligned device
// allocation, so byte offset off[i] fixes message i's alignment); every
// off[i] + len[i] <= msg_bytes is checked here, before anything is launched
int ntp_hram(uint64_t n, const uint32_t* R8, const uint32_t* A8, const uint8_t* msg, uint64_t msg_bytes,
             const uint64_t* off, const uint64_t* len, uint32_t* out8, int fast) {
  for (uint64_t i = 0; i < n; ++i)
    if (!msg_slice(off[i], len[i], msg_bytes).ok) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  // load_words reads whole 4-byte granules: keep the allocation a multiple of 16 past the end
  const size_t padded = (size_t)((msg_bytes + 15) / 16 * 16 + 16);
  Dev dR(&err, R8, 32 * n), dA(&err, A8, 32 * n), dm(&err, nullptr, padded), doff(&err, off, 8 * n),
      dlen(&err, len, 8 * n), dout(&err, nullptr, 32 * n);
  if (err == hipSuccess) err = hipMemset(dm.p, 0, padded);
  if (err == hipSuccess && msg_bytes) err = hipMemcpy(dm.p, msg, msg_bytes, hipMemcpyHostToDevice);
  if (fast) {
    NTP_LAUNCH(k_hram<true>, dR.as<uint32_t>(), dA.as<uint32_t>(), dm.as<uint8_t>(), doff.as<uint64_t>(),
               dlen.as<uint64_t>(), dout.as<uint32_t>())
  } else {
    NTP_LAUNCH(k_hram<false>, dR.as<uint32_t>(), dA.as<uint32_t>(), dm.as<uint8_t>(), doff.as<uint64_t>(),
               dlen.as<uint64_t>(), dout.as<uint32_t>())
  }
  dout.back(out8, 32 * n);
  return (int)err;
}
int ntp_point_checks(uint64_t n, const uint32_t* enc8, uint32_t* out4) {
  NTP_BEGIN
  Dev de(&err, enc8, 32 * n), dout(&err, nullptr, 16 * n);
  NTP_LAUNCH(k_point_checks, de.as<uint32_t>(), dout.as<uint32_t>())
  dout.back(out4, 16 * n);
  return (int)err;
}
int ntp_ladder_uv(uint64_t n, const uint32_t* A8, const uint32_t* R8, const uint32_t* u8, const uint32_t* uneg,
                  const uint32_t* v8, const int32_t* bits, uint32_t* out8) {
  NTP_BEGIN
  for (uint64_t i = 0; i < n; ++i)  // 4 W <= 256 digits of the recoded strings
    if (bits[i] < 0 || bits[i] > 253) return (int)hipErrorInvalidValue;
  const size_t ws_bytes = (size_t)grid(n) * kBlock * kAEntries * kAQuads * sizeof(uint4);
  Dev dA(&err, A8, 32 * n), dR(&err, R8, 32 * n), du(&err, u8, 32 * n), dn(&err, uneg, 4 * n), dv(&err, v8, 32 * n),
      db(&err, bits, 4 * n), dws(&err, nullptr, ws_bytes), dout(&err, nullptr, 32 * n);
  NTP_LAUNCH(k_ladder_uv, dA.as<uint32_t>(), dR.as<uint32_t>(), du.as<uint32_t>(), dn.as<uint32_t>(),
             dv.as<uint32_t>(), db.as<int32_t>(), dws.as<uint4>(), dout.as<uint32_t>())
  dout.back(out8, 32 * n);
  return (int)err;
}
int ntp_sc_unbalanced(uint64_t n, const uint32_t* k8, uint32_t* u8, uint32_t* uneg, uint32_t* v8, int32_t* ubits,
                      int32_t* vbits, int lehmer) {
  NTP_BEGIN
  Dev dk(&err, k8, 32 * n), du(&err, nullptr, 32 * n), dn(&err, nullptr, 4 * n), dv(&err, nullptr, 32 * n),
      dub(&err, nullptr, 4 * n), dvb(&err, nullptr, 4 * n);
  if (lehmer) {
    NTP_LAUNCH(k_sc_unbalanced<true>, dk.as<uint32_t>(), du.as<uint32_t>(), dn.as<uint32_t>(), dv.as<uint32_t>(),
               dub.as<int32_t>(), dvb.as<int32_t>())
  } else {
    NTP_LAUNCH(k_sc_unbalanced<false>, dk.as<uint32_t>(), du.as<uint32_t>(), dn.as<uint32_t>(), dv.as<uint32_t>(),
               dub.as<int32_t>(), dvb.as<int32_t>())
  }
  du.back(u8, 32 * n);
  dn.back(uneg, 4 * n);
  dv.back(v8, 32 * n);
  dub.back(ubits, 4 * n);
  dvb.back(vbits, 4 * n);
  return (int)err;
}
// blob: the key table, ntp::ktab_probe_bytes(capacity) bytes (see DevBlob); one launch per call
int ntp_ktab_fill(uint64_t n, const uint32_t* A8, uint8_t* blob, uint32_t capacity, uint32_t* slot) {
  if (capacity < 1 || capacity > ntp::kKtProbeMaxCap) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  Dev dA(&err, A8, 32 * n), ds(&err, nullptr, 4 * n);
  DevBlob db(&err, blob, capacity);
  NTP_LAUNCH(k_ktab_fill, dA.as<uint32_t>(), db.d.as<uint32_t>(), capacity, ds.as<uint32_t>())
  ds.back(slot, 4 * n);
  db.back();
  return (int)err;
}
int ntp_ktab_point(uint64_t n, const uint32_t* A8, const int32_t* td2, uint8_t* blob, uint32_t capacity,
                   uint32_t* out3, uint32_t* enc8) {
  if (capacity < 1 || capacity > ntp::kKtProbeMaxCap || !ntp::ktab_point_args_ok(n, td2)) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  Dev dA(&err, A8, 32 * n), dt(&err, td2, 8 * n), do3(&err, nullptr, 12 * n), de(&err, nullptr, 32 * n);
  DevBlob db(&err, blob, capacity);
  NTP_LAUNCH(k_ktab_point, dA.as<uint32_t>(), dt.as<int32_t>(), db.d.as<uint32_t>(), capacity, do3.as<uint32_t>(),
             de.as<uint32_t>())
  do3.back(out3, 12 * n);
  de.back(enc8, 32 * n);
  db.back();
  return (int)err;
}
int ntp_ladder_uv3(uint64_t n, const uint32_t* kidx, const uint32_t* R8, const uint32_t* u8, const uint32_t* v8,
                   const uint32_t* sc4, uint8_t* blob, uint32_t capacity, uint32_t* out8) {
  if (capacity < 1 || capacity > ntp::kKtProbeMaxCap || !ntp::ladder_uv3_args_ok(n, kidx, sc4, capacity))
    return (int)hipErrorInvalidValue;
  NTP_BEGIN
  const size_t ws_bytes = (size_t)grid(n) * kBlock * kAEntries * kAQuads * sizeof(uint4);
  Dev dk(&err, kidx, 4 * n), dR(&err, R8, 32 * n), du(&err, u8, 32 * n), dv(&err, v8, 32 * n), ds(&err, sc4, 16 * n),
      dws(&err, nullptr, ws_bytes), dout(&err, nullptr, 32 * n);
  DevBlob db(&err, blob, capacity);
  NTP_LAUNCH(k_ladder_uv3, dk.as<uint32_t>(), dR.as<uint32_t>(), du.as<uint32_t>(), dv.as<uint32_t>(),
             ds.as<uint32_t>(), db.d.as<uint32_t>(), capacity, dws.as<uint4>(), dout.as<uint32_t>())
  dout.back(out8, 32 * n);
  db.back();
  return (int)err;
}

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
int ntp_wcomb_digits(int bits, uint64_t n, const uint32_t* x8, uint32_t* out) {
  if (!ntp::wcomb_width(bits, [](auto) {})) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  Dev dx(&err, x8, 32 * n), dout(&err, nullptr, 4 * ntp::kWcDigitWords * n);
  ntp::wcomb_width(bits, [&](auto w) {
    NTP_LAUNCH(k_wcomb_digits<decltype(w)::value>, dx.as<uint32_t>(), dout.as<uint32_t>())
  });
  dout.back(out, 4 * ntp::kWcDigitWords * n);
  return (int)err;
}
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

// ---- the key-table cache's comb path.  blob: ntp::kcomb_probe_bytes(capacity) bytes -- control
// block, index, pool entries, comb pool, guard -- prefilled by the caller; entry indices, scalars
// (k < 2^253) and modes are checked here, on the host, before anything is launched.
int ntp_kcomb_fill(uint64_t n, const uint32_t* A8, uint8_t* blob, uint32_t capacity, uint32_t* slot) {
  if (!ntp::kcomb_cap_ok(capacity)) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  const size_t ws_bytes = (size_t)grid(n) * kBlock * kAEntries * kAQuads * sizeof(uint4);
  Dev dA(&err, A8, 32 * n), ds(&err, nullptr, 4 * n), dws(&err, nullptr, ws_bytes);
  DevBlob db(&err, blob, capacity, true);
  NTP_LAUNCH(k_kcomb_fill, dA.as<uint32_t>(), db.d.as<uint32_t>(), capacity, dws.as<uint4>(), ds.as<uint32_t>())
  ds.back(slot, 4 * n);
  db.back();
  return (int)err;
}
// line[i]: any number (comb_line clamps it to the last line)
int ntp_kcomb_line(uint64_t n, const uint32_t* A8, const uint32_t* line, uint8_t* blob, uint32_t capacity, uint32_t* out3,
                   uint32_t* limbs30) {
  if (!ntp::kcomb_cap_ok(capacity)) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  Dev dA(&err, A8, 32 * n), dl(&err, line, 4 * n), do3(&err, nullptr, 12 * n), dq(&err, nullptr, 120 * n);
  DevBlob db(&err, blob, capacity, true);
  NTP_LAUNCH(k_kcomb_line, dA.as<uint32_t>(), dl.as<uint32_t>(), db.d.as<uint32_t>(), capacity, do3.as<uint32_t>(),
             dq.as<uint32_t>())
  do3.back(out3, 12 * n);
  dq.back(limbs30, 120 * n);
  db.back();
  return (int)err;
}
int ntp_kc_picks(uint64_t n, const uint32_t* k8, uint32_t* out65) {
  if (!ntp::kc_scalars_ok(n, k8)) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  Dev dk(&err, k8, 32 * n), dout(&err, nullptr, 4 * ntp::kKcPickWords * n);
  NTP_LAUNCH(k_kc_picks, dk.as<uint32_t>(), dout.as<uint32_t>())
  dout.back(out65, 4 * ntp::kKcPickWords * n);
  return (int)err;
}
int ntp_ladder_kc(uint64_t n, const uint32_t* kidx, const uint32_t* k8, const uint32_t* dead, uint8_t* blob,
                  uint32_t capacity, uint32_t* out8) {
  if (!ntp::kcomb_cap_ok(capacity) || !ntp::ladder_kc_args_ok(n, kidx, k8, dead, capacity)) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  Dev di(&err, kidx, 4 * n), dk(&err, k8, 32 * n), dd(&err, dead, 4 * n), dout(&err, nullptr, 32 * n);
  DevBlob db(&err, blob, capacity, true);
  NTP_LAUNCH(k_ladder_kc, di.as<uint32_t>(), dk.as<uint32_t>(), dd.as<uint32_t>(), db.d.as<uint32_t>(), capacity,
             dout.as<uint32_t>())
  dout.back(out8, 32 * n);
  db.back();
  return (int)err;
}
int ntp_compare_one(uint64_t n, const uint32_t* x8, const uint32_t* y8, const uint32_t* z8, const uint32_t* R8,
                    const uint32_t* mode, uint32_t* out1) {
  if (!ntp::modes_ok(n, mode)) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  Dev dx(&err, x8, 32 * n), dy(&err, y8, 32 * n), dz(&err, z8, 32 * n), dR(&err, R8, 32 * n), dm(&err, mode, 4 * n),
      dout(&err, nullptr, 4 * n);
  NTP_LAUNCH(k_compare_one, dx.as<uint32_t>(), dy.as<uint32_t>(), dz.as<uint32_t>(), dR.as<uint32_t>(), dm.as<uint32_t>(),
             dout.as<uint32_t>())
  dout.back(out1, 4 * n);
  return (int)err;
}
// the comb of B: key 0 of the live comb set, which must be the narrowest width (ntp_wcomb_build
// of B alone, not negated); any 256-bit s stays inside that table
int ntp_verify_kc(uint64_t n, const uint32_t* kidx, const uint32_t* kflags, const uint32_t* R8, const uint32_t* S8,
                  const uint32_t* k8, const uint32_t* mode, uint8_t* blob, uint32_t capacity, uint32_t* out1) {
  if (!g_wc.p || g_wc.bits != kKeyCombNarrow || !ntp::kcomb_cap_ok(capacity) ||
      !ntp::verify_kc_args_ok(n, kidx, kflags, k8, mode, capacity))
    return (int)hipErrorInvalidValue;
  for (uint64_t i = 0; i < n; ++i)
    if (!ntp::wcomb_scalar_ok<kKeyCombNarrow>(S8 + 8 * i)) return (int)hipErrorInvalidValue;
  NTP_BEGIN
  Dev di(&err, kidx, 4 * n), df(&err, kflags, 4 * n), dR(&err, R8, 32 * n), dS(&err, S8, 32 * n), dk(&err, k8, 32 * n),
      dm(&err, mode, 4 * n), dout(&err, nullptr, 4 * n);
  DevBlob db(&err, blob, capacity, true);
  NTP_LAUNCH(k_verify_kc<kKeyCombNarrow>, (const uint32_t*)g_wc.p, di.as<uint32_t>(), df.as<uint32_t>(), dR.as<uint32_t>(),
             dS.as<uint32_t>(), dk.as<uint32_t>(), dm.as<uint32_t>(), db.d.as<uint32_t>(), capacity, dout.as<uint32_t>())
  dout.back(out1, 4 * n);
  db.back();
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
