// calibrate.cpp -- calibration of the small-call cost model (nt_set_small_call_path).
#include <chrono>

#include "cpu_lane.hpp"
#include "runtime.hpp"

namespace ntrt {

// Host lane: verify_strict of the RFC 8032 section 7.1 TEST 1 vector (a valid
// signature over the empty message) and SHA-512 of 1 MiB, on the calling
// thread; the pool wake-up from a no-op call on `threads` threads.  GPU: one
// signature through nt_ed25519_verify_strict (below one round: the launch +
// copy floor), a 64-byte digest (the digest call floor) and a 1 MiB digest
// (one lane's serial chain), medians of a few calls after a warm-up.
// NT_SMALL_* variables override single fields afterwards.
static double median_of(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int calibrate_small(nt_ctx* ctx) {
  using clk = std::chrono::steady_clock;
  auto us = [](clk::time_point a) { return std::chrono::duration<double, std::micro>(clk::now() - a).count(); };
  static const uint8_t kPk[32] = {0xd7, 0x5a, 0x98, 0x01, 0x82, 0xb1, 0x0a, 0xb7, 0xd5, 0x4b, 0xfe,
                                  0xd3, 0xc9, 0x64, 0x07, 0x3a, 0x0e, 0xe1, 0x72, 0xf3, 0xda, 0xa6,
                                  0x23, 0x25, 0xaf, 0x02, 0x1a, 0x68, 0xf7, 0x07, 0x51, 0x1a};
  static const uint8_t kSig[64] = {0xe5, 0x56, 0x43, 0x00, 0xc3, 0x60, 0xac, 0x72, 0x90, 0x86, 0xe2, 0xcc, 0x80,
                                   0x6e, 0x82, 0x8a, 0x84, 0x87, 0x7f, 0x1e, 0xb8, 0xe5, 0xd9, 0x74, 0xd8, 0x73,
                                   0xe0, 0x65, 0x22, 0x49, 0x01, 0x55, 0x5f, 0xb8, 0x82, 0x15, 0x90, 0xa3, 0x3b,
                                   0xac, 0xc6, 0x1e, 0x39, 0x70, 0x1c, 0xf9, 0xb4, 0x6b, 0xd2, 0x5b, 0xf5, 0xf0,
                                   0x59, 0x5b, 0xbe, 0x24, 0x65, 0x51, 0x41, 0x43, 0x8e, 0x7a, 0x10, 0x0b};
  static const uint8_t kEmpty[1] = {0};
  NtSmallModel m;
  // host lane, one thread
  bool ok = nt::cpu::verify(nt::kStrict, kPk, kSig, kEmpty, 0);
  {
    std::vector<double> t;
    for (int r = 0; r < 5; ++r) {
      const auto a = clk::now();
      for (int k = 0; k < 8; ++k) ok &= nt::cpu::verify(nt::kStrict, kPk, kSig, kEmpty, 0);
      t.push_back(us(a) / 8);
    }
    if (!ok) return NT_EHIP;  // the host lane must accept a known-good signature
    m.cpu_verify_us = median_of(t);
  }
  std::vector<uint8_t> big(1u << 20, 0x5a);
  {
    uint8_t d[32];
    std::vector<double> t;
    for (int r = 0; r < 3; ++r) {
      const auto a = clk::now();
      nt::cpu::sha512_trunc32(big.data(), big.size(), d);
      t.push_back(us(a));
    }
    m.cpu_sha_mbs = (double)big.size() / median_of(t);  // bytes per us = MB/s
  }
  {
    const int T = std::max(1, ctx->small_threads.load());
    std::vector<double> t;
    for (int r = 0; r < 7; ++r) {
      const auto a = clk::now();
      nt::cpu::parallel_for((uint64_t)T, T, [](uint64_t) {});
      t.push_back(us(a));
    }
    m.spawn_us = T > 1 ? median_of(t) : 0.0;
  }
  // GPU floors (the caller set small_mode = OFF: these calls run the kernels)
  {
    // gpu_verify_us is the UNCACHED kernel's floor (small_model.hpp): the repetitions below use one
    // key, which the key-table cache would serve from its third sighting on -- and a cached lone
    // verify, with no square root of R and half the ladder, is no measure of a call whose keys are
    // new.  The cache is kept out of these launches.
    struct KtabPause {
      nt_ctx* c;
      explicit KtabPause(nt_ctx* x) : c(x) { for (auto& d : c->devs) d->ktab_paused.fetch_add(1); }
      ~KtabPause() { for (auto& d : c->devs) d->ktab_paused.fetch_sub(1); }
    } pause(ctx);
    const uint64_t off = 0, len = 0;
    uint8_t bm = 0;
    std::vector<double> t;
    for (int r = 0; r < 6; ++r) {
      const auto a = clk::now();
      NT_CHK0(nt_ed25519_verify_strict(ctx, kPk, kSig, kEmpty, &off, &len, 1, &bm));
      if (r) t.push_back(us(a));
    }
    if (!(bm & 1)) return NT_EHIP;
    m.gpu_verify_us = median_of(t);
  }
  {
    // the key-cache kernel's floor: one signature through a one-key set (16-bit
    // key combs, 67 MB, freed after; the floor is the launch and one lane's
    // serial chain -- 27 comb additions and an inversion -- whatever the width)
    nt_keyset* ks = nullptr;
    NT_CHK0(keyset_create(ctx, kPk, 1, nt::kKeyCombNarrow, &ks));
    const uint64_t off = 0, len = 0;
    const uint32_t k0 = 0;
    uint8_t bm = 0;
    std::vector<double> t;
    int rc = NT_OK;
    for (int r = 0; r < 6 && rc == NT_OK; ++r) {
      const auto a = clk::now();
      rc = nt_ed25519_verify_keyset(ctx, ks, NT_MODE_STRICT, &k0, kSig, kEmpty, &off, &len, 1, &bm);
      if (r) t.push_back(us(a));
    }
    nt_keyset_free(ks);
    if (rc != NT_OK) return rc;
    if (!(bm & 1)) return NT_EHIP;
    m.gpu_keyset_us = median_of(t);
  }
  {
    uint8_t d[32];
    const uint64_t off = 0, len64 = 64, len1m = big.size();
    std::vector<double> ts, tb;
    for (int r = 0; r < 6; ++r) {
      auto a = clk::now();
      NT_CHK0(nt_sha512_trunc32(ctx, big.data(), &off, &len64, 1, d));
      if (r) ts.push_back(us(a));
    }
    for (int r = 0; r < 3; ++r) {
      auto a = clk::now();
      NT_CHK0(nt_sha512_trunc32(ctx, big.data(), &off, &len1m, 1, d));
      if (r) tb.push_back(us(a));
    }
    m.gpu_call_us = median_of(ts);
    const double lane = median_of(tb) - m.gpu_call_us - (double)big.size() / (m.pcie_gbs * 1e3);
    m.gpu_lane_mbs = (double)big.size() / std::max(lane, 1.0);
  }
  m.calibrated = 1;
  ctx->small_model = small_model_with_env(m);
  return NT_OK;
}

}  // namespace ntrt
