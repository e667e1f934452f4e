// keyset.cpp -- the committee key cache's lifecycle: nt_keyset_create / free / flags / info.
#include "runtime.hpp"

namespace ntrt {

// Small-call path: key encoding and check mode of one key-cache entry, as
// the key-cache kernel's loader decodes key_idx (k_keyset.inc KsLoader): in
// NT_MODE_MIXED bit 31 selects strict; an index >= nkeys is no key (-1, reject).
int keyset_key(const nt_keyset* ks, int mode, uint32_t kraw, uint8_t A[32]) {
  int m = mode == NT_MODE_STRICT ? nt::kStrict : nt::kCofactorless;
  if (mode == NT_MODE_MIXED) {
    m = (kraw & NT_KEY_STRICT_BIT) ? nt::kStrict : nt::kCofactorless;
    kraw &= ~NT_KEY_STRICT_BIT;
  }
  if (kraw >= ks->nkeys) return -1;
  std::memcpy(A, ks->enc.data() + 32ull * kraw, 32);
  return m;
}

// nt_keyset_create at a given key-comb width (0 = the widest that fits)
int keyset_create(nt_ctx* ctx, const uint8_t* pk32, uint32_t nkeys, int bits, nt_keyset** out) {
  if (!ctx || !out || (nkeys && !pk32)) return NT_EINVAL;
  *out = nullptr;
  // verification against the set reads the comb of B: it takes its share of the
  // budget first, the key combs get what is left
  for (auto& d : ctx->devs) {
    std::lock_guard<std::mutex> lk(d->mu);
    NT_CHK(comb_b_for(*d));
  }
  auto ks = std::make_unique<nt_keyset>();
  ks->ctx = ctx;
  ks->nkeys = nkeys;
  ks->bits = bits ? bits : keyset_comb_bits(ctx, nkeys);
  if (ks->bits == 0) return NT_ENOMEM;
  ks->flags.assign(nkeys, 0);
  if (nkeys) ks->enc.assign(pk32, pk32 + 32ull * nkeys);
  ks->t = std::make_shared<KsTables>();
  KsTables& T = *ks->t;
  T.nkeys = nkeys;
  T.bits = ks->bits;
  T.dev.resize(ctx->devs.size());
  for (size_t di = 0; di < ctx->devs.size(); ++di) {
    Device& dv = *ctx->devs[di];
    std::lock_guard<std::mutex> lk(dv.mu);
    NT_TRY(hipSetDevice(dv.ordinal));
    auto& pd = T.dev[di];
    pd.ordinal = dv.ordinal;
    const size_t nk = std::max<uint32_t>(nkeys, 1);
    const uint64_t comb = nt::wcomb_bytes_per_key(ks->bits) * nk;
    if (!dv.budget->reserve(comb)) return NT_ENOMEM;
    pd.budget = dv.budget;
    pd.reserved = comb;
    if (hipMalloc(&pd.d_enc, 32 * nk) != hipSuccess) return NT_ENOMEM;
    if (hipMalloc(&pd.d_meta, 4 * nk) != hipSuccess) return NT_ENOMEM;
    if (table_malloc((void**)&pd.d_comb, comb) != hipSuccess) {
      (void)hipGetLastError();
      pd.d_comb = nullptr;
      return NT_ENOMEM;
    }
    if (nkeys) {
      NT_TRY(hipMemcpyAsync(pd.d_enc, pk32, 32ull * nkeys, hipMemcpyHostToDevice, dv.lane[0].stream));
      NT_TRY(hipStreamSynchronize(dv.lane[0].stream));
      const int rc = dv.build_wcombs(ks->bits, (const uint32_t*)pk32, nkeys, 1, pd.d_comb, pd.d_meta);
      if (rc != NT_OK) return rc;
      if (di == 0)
        NT_TRY(hipMemcpyAsync(ks->flags.data(), pd.d_meta, 4ull * nkeys, hipMemcpyDeviceToHost, dv.lane[0].stream));
    }
    NT_TRY(hipStreamSynchronize(dv.lane[0].stream));
  }
  *out = ks.release();
  return NT_OK;
}

}  // namespace ntrt

using namespace ntrt;

extern "C" {

int nt_keyset_create(nt_ctx* ctx, const uint8_t* pk32, uint32_t nkeys, nt_keyset** out) {
  // the widest width that fits, or -- when hipMalloc refuses it (another process on the
  // device may take the memory between the check and the allocation) -- the next narrower
  const int b = keyset_comb_bits(ctx, nkeys);
  if (b == 0 || std::getenv("NT_KEYSET_COMB_BITS")) return keyset_create(ctx, pk32, nkeys, b, out);
  int rc = NT_ENOMEM;
  for (const int w : {nt::kKeyCombReduced, nt::kKeyCombWide, nt::kKeyCombMid, nt::kKeyCombNarrow}) {
    if (w > b) continue;
    rc = keyset_create(ctx, pk32, nkeys, w, out);
    if (rc != NT_ENOMEM) return rc;
  }
  return rc;
}

void nt_keyset_free(nt_keyset* ks) { delete ks; }

int nt_keyset_flags(const nt_keyset* ks, uint32_t i, uint32_t* flags) {
  if (!ks || !flags || i >= ks->nkeys) return NT_EINVAL;
  *flags = ks->flags[i];
  return NT_OK;
}

int nt_keyset_info(const nt_keyset* ks, uint32_t* comb_bits, uint64_t* bytes_per_device) {
  if (!ks) return NT_EINVAL;
  const uint64_t nk = std::max<uint32_t>(ks->nkeys, 1);
  if (comb_bits) *comb_bits = (uint32_t)ks->bits;
  if (bytes_per_device) *bytes_per_device = (nt::wcomb_bytes_per_key(ks->bits) + 36) * nk;
  return NT_OK;
}

}  // extern "C"
