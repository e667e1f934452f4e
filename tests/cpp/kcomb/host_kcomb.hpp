// host_kcomb.hpp -- TEST INFRASTRUCTURE: the host key-table cache (../ktab/host_ktab.hpp, included
// and left as it is) with the second pool holding the keys' combs, laid out like the device's
// (kernels_common.hpp DevKTab with kComb): cap x kKtCombBytes, 33 lines of 128 bytes per entry
// index, 30 words of each used.  comb == nullptr is "no comb": has_comb() says so, nothing below
// is called, and the policy builds and verifies as HostKTab does.
#pragma once
#include "../ktab/host_ktab.hpp"

struct HostKComb : HostKTab {
  static constexpr bool kComb = true;
  uint8_t* comb;  // cap combs, or nullptr
  HostKComb(uint64_t* slots_, uint32_t smask_, uint8_t* pool_, uint32_t cap_, uint32_t* ctl_, uint8_t* comb_)
      : HostKTab{slots_, smask_, pool_, cap_, ctl_}, comb(comb_) {}
  bool has_comb() const { return comb != nullptr; }
  uint32_t* comb_line(uint32_t idx, uint32_t entry) const {
    return (uint32_t*)(comb + (size_t)idx * nt::kKtCombBytes + (size_t)(entry < nt::kKcEntries ? entry : nt::kKcEntries - 1u) * nt::kKcLineBytes);
  }
  void comb_store(uint32_t idx, uint32_t entry, const nt::ge_niels& q) const {
    uint32_t* p = comb_line(idx, entry);
    for (int i = 0; i < 10; ++i) {
      p[i] = q.ypx.v[i]; p[10 + i] = q.ymx.v[i]; p[20 + i] = q.xy2d.v[i];
    }
  }
  void comb_load(uint32_t idx, uint32_t entry, nt::ge_niels& q) const {
    const uint32_t* p = comb_line(idx, entry);
    for (int i = 0; i < 10; ++i) {
      q.ypx.v[i] = p[i]; q.ymx.v[i] = p[10 + i]; q.xy2d.v[i] = p[20 + i];
    }
  }
};
