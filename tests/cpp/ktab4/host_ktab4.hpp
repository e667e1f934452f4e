// host_ktab4.hpp -- TEST INFRASTRUCTURE: the host key-table cache (../ktab/host_ktab.hpp,
// included and left as it is) with the extension pool of the fourth table, laid out like the
// device's (kernels_common.hpp DevKTab): cap x kKtExtBytes, 8 points of 40 words per entry
// index.  ext == nullptr is "no fourth table": has_ext() says so and nothing below is called.
#pragma once
#include "../ktab/host_ktab.hpp"

struct HostKTab4 : HostKTab {
  static constexpr bool kExt = true;
  uint8_t* ext;  // cap fourth tables, or nullptr
  HostKTab4(uint64_t* slots_, uint32_t smask_, uint8_t* pool_, uint32_t cap_, uint32_t* ctl_, uint8_t* ext_)
      : HostKTab{slots_, smask_, pool_, cap_, ctl_}, ext(ext_) {}
  bool has_ext() const { return ext != nullptr; }
  uint32_t* ext_point(uint32_t idx, uint32_t j) const {
    return (uint32_t*)(ext + (size_t)idx * nt::kKtExtBytes) + (size_t)((j - 1u) & 7u) * 40;
  }
  void ext_store(uint32_t idx, uint32_t j, const nt::ge_cached& c) const {
    uint32_t* p = ext_point(idx, j);
    for (int i = 0; i < 10; ++i) {
      p[i] = c.YpX.v[i]; p[10 + i] = c.YmX.v[i]; p[20 + i] = c.Z2.v[i]; p[30 + i] = c.T2d.v[i];
    }
  }
  void ext_load_signed(uint32_t idx, int32_t d, nt::ge_cached& c) const {
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    const uint32_t* p = ext_point(idx, a);
    for (int i = 0; i < 10; ++i) {
      c.YpX.v[i] = p[i]; c.YmX.v[i] = p[10 + i]; c.Z2.v[i] = p[20 + i]; c.T2d.v[i] = p[30 + i];
    }
    nt::ge_cached_cneg(c, d < 0);
    if (a == 0) nt::ge_cached_0(c);  // entry 0 is synthesized
  }
};
