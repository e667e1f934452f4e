// host_ktab.hpp -- TEST INFRASTRUCTURE: the key-table cache of the verify kernel
// (ktab.hpp) over plain host memory with host atomics, laid out like
// the device's (kernels_common.hpp DevKTab): 8-byte index slots, pool entries of
// kKtEntryBytes (128-B header: 8 tag words + flags; then 3 x 8 points of 40
// words), a control block {bump counter, fast rows, builds, old-path rows}.
// Shared by the ctypes harness (nt_ktab_harness.cpp) and the threaded protocol
// program (ktab_threads.cpp).
#pragma once
#include <cstdint>
#include <cstring>

#include "../../../narwhal-tusk_amd/csrc/ed25519_ops.hpp"

struct HostKTab {
  static constexpr bool kEnabled = true;
  uint64_t* slots;  // smask + 1 of them
  uint32_t smask;
  uint8_t* pool;    // cap entries
  uint32_t cap;
  uint32_t* ctl;    // 4 words
  mutable uint32_t dig[16] = {};         // the digit words of the verification in flight
  mutable uint32_t claim = 0xffffffffu;  // the claimed slot of the verification in flight
  bool active() const { return slots != nullptr; }
  uint32_t slot_mask() const { return smask; }
  uint32_t capacity() const { return cap; }
  // the slot words carry the hand-off: acquire loads, release publish (the device
  // form: relaxed loads + ONE acquire fence, drain + release fence + relaxed store)
  uint64_t slot_load(uint32_t i) const { return __atomic_load_n(slots + (i & smask), __ATOMIC_ACQUIRE); }
  uint64_t slot_cas(uint32_t i, uint64_t expect, uint64_t desired) const {  // returns the word found
    __atomic_compare_exchange_n(slots + (i & smask), &expect, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expect;
  }
  void dig_put(uint32_t i, uint32_t w) const { dig[i & 15u] = w; }
  uint32_t dig_get(uint32_t i) const { return dig[i & 15u]; }
  void claim_put(uint32_t v) const { claim = v; }
  uint32_t claim_get() const { return claim; }
  void slot_store(uint32_t i, uint64_t w) const { __atomic_store_n(slots + (i & smask), w, __ATOMIC_RELAXED); }
  void slot_publish(uint32_t i, uint64_t w) const { __atomic_store_n(slots + (i & smask), w, __ATOMIC_RELEASE); }
  void acquire() const { __atomic_thread_fence(__ATOMIC_ACQUIRE); }
  void drain_release() const { __atomic_thread_fence(__ATOMIC_RELEASE); }
  uint32_t pool_used() const { return __atomic_load_n(ctl, __ATOMIC_RELAXED); }
  uint32_t pool_take() const { return __atomic_fetch_add(ctl, 1u, __ATOMIC_RELAXED); }
  void count(int which) const { __atomic_fetch_add(ctl + 1 + which, 1u, __ATOMIC_RELAXED); }
  uint32_t* entry(uint32_t idx) const { return (uint32_t*)(pool + (size_t)idx * nt::kKtEntryBytes); }
  uint32_t* point(uint32_t idx, uint32_t t, uint32_t j) const {
    return entry(idx) + nt::kKtHeaderBytes / 4 + (size_t)((t % nt::kKtTables) * nt::kKtPerTable + ((j - 1u) & 7u)) * 40;
  }
  void hdr_load(uint32_t idx, uint32_t tag[8], uint32_t& flags) const {
    const uint32_t* e = entry(idx);
    std::memcpy(tag, e, 32);
    flags = e[8];
  }
  void hdr_store(uint32_t idx, const uint32_t tag[8], uint32_t flags) const {
    uint32_t* e = entry(idx);
    std::memcpy(e, tag, 32);
    e[8] = flags;
  }
  void tab_store(uint32_t idx, uint32_t t, uint32_t j, const nt::ge_cached& c) const {
    uint32_t* p = point(idx, t, j);
    for (int i = 0; i < 10; ++i) {
      p[i] = c.YpX.v[i]; p[10 + i] = c.YmX.v[i]; p[20 + i] = c.Z2.v[i]; p[30 + i] = c.T2d.v[i];
    }
  }
  void tab_load_signed(uint32_t idx, uint32_t t, int32_t d, nt::ge_cached& c) const {
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    const uint32_t* p = point(idx, t, a);
    for (int i = 0; i < 10; ++i) {
      c.YpX.v[i] = p[i]; c.YmX.v[i] = p[10 + i]; c.Z2.v[i] = p[20 + i]; c.T2d.v[i] = p[30 + i];
    }
    nt::ge_cached_cneg(c, d < 0);
    if (a == 0) nt::ge_cached_0(c);  // entry 0 is synthesized
  }
};
