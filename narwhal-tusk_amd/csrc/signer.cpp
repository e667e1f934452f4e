// signer.cpp -- the signer bound to a node's own key (include/ntsigner.h): nts_signer_*,
// nts_sign_digests, nts_votes_sign, nts_dev_votes_sign.  One H2D copy per input array, one
// launch (k_signer.hip), D2H copies; small calls run the same signer_ops.hpp functions on the
// host lane whenever a key-cache verification of that size would.
#include "../../include/ntsigner.h"
#include "pipeline.hpp"

using namespace ntrt;

constexpr size_t kKeyBytes = 192;  // signer_ops.hpp SignerKey

struct nts_signer {
  nt_ctx* ctx = nullptr;
  uint8_t key[kKeyBytes] = {};  // the host copy
  std::vector<void*> d_key;     // one record per device entry of ctx
};

namespace {

// volatile: the stores outlive the object they clear
void wipe(uint8_t* p, size_t n) {
  volatile uint8_t* v = p;
  for (size_t i = 0; i < n; ++i) v[i] = 0;
}

bool usable(const nt_ctx* ctx, const nts_signer* s) { return ctx && s && s->ctx == ctx; }

}  // namespace

extern "C" {

int nts_signer_create(nt_ctx* ctx, const uint8_t seed32[32], nts_signer** out) {
  if (!ctx || !seed32 || !out) return NT_EINVAL;
  *out = nullptr;
  nt::cpu::init(std::max(1, ctx->small_threads.load()));  // the host comb of B: the key record is made here
  std::unique_ptr<nts_signer> s(new nts_signer);
  s->ctx = ctx;
  nt::cpu::signer_key(seed32, s->key);
  s->d_key.assign(ctx->devs.size(), nullptr);
  int rc = NT_OK;
  for (size_t d = 0; d < ctx->devs.size() && rc == NT_OK; ++d) {
    if (hipSetDevice(ctx->devs[d]->ordinal) != hipSuccess) rc = NT_EHIP;
    else if (hipMalloc(&s->d_key[d], kKeyBytes) != hipSuccess) {
      (void)hipGetLastError();
      s->d_key[d] = nullptr;
      rc = NT_ENOMEM;
    } else if (hipMemcpy(s->d_key[d], s->key, kKeyBytes, hipMemcpyHostToDevice) != hipSuccess) rc = NT_EHIP;
  }
  if (rc != NT_OK) {
    nts_signer_free(s.release());
    return rc;
  }
  *out = s.release();
  return NT_OK;
}

void nts_signer_free(nts_signer* s) {
  if (!s) return;
  for (size_t d = 0; d < s->d_key.size(); ++d) {
    if (!s->d_key[d]) continue;
    (void)hipSetDevice(s->ctx->devs[d]->ordinal);
    (void)hipMemset(s->d_key[d], 0, kKeyBytes);  // hipFree waits for it
    (void)hipFree(s->d_key[d]);
  }
  wipe(s->key, kKeyBytes);
  delete s;
}

int nts_signer_public(const nts_signer* s, uint8_t pk32[32]) {
  if (!s || !pk32) return NT_EINVAL;
  std::memcpy(pk32, s->key + 96, 32);  // SignerKey::A
  return NT_OK;
}

int nts_sign_digests(nt_ctx* ctx, const nts_signer* s, const uint8_t* digest32, uint64_t n, uint8_t* sig64) {
  if (!usable(ctx, s)) return NT_EINVAL;
  if (n == 0) return NT_OK;
  if (!digest32 || !sig64) return NT_EINVAL;
  if (small_verify(ctx, n, nt::kRouteKeyCache)) {
    nt::cpu::parallel_for(n, small_threads(ctx, n), [&](uint64_t i) {
      nt::cpu::sign_fixed(s->key, digest32 + 32 * i, sig64 + 64 * i);
    });
    ctx->calls_host++;
    return NT_OK;
  }
  ctx->calls_gpu++;
  return run_sharded(ctx, n, 64, [&](Device& dv, uint64_t lo, uint64_t hi) -> int {
    NT_CHK(comb_b_for(dv));
    const uint64_t m = hi - lo;
    hipStream_t st = dv.lane[0].stream;
    NT_CHK(dv.d[B_DATA].ensure(m * 32));
    NT_CHK(dv.d[B_SIG].ensure(m * 64));
    NT_TRY(hipMemcpyAsync(dv.d[B_DATA].p, digest32 + 32 * lo, m * 32, hipMemcpyHostToDevice, st));
    NT_TRY(nt::launch_signer_digests(s->d_key[dv.group], dv.d[B_DATA].as<uint8_t>(), m, dv.d_combB, dv.bbits,
                                     dv.d[B_SIG].as<uint8_t>(), dv.sign_blocks, st));
    NT_TRY(hipMemcpyAsync(sig64 + 64 * lo, dv.d[B_SIG].p, m * 64, hipMemcpyDeviceToHost, st));
    NT_TRY(hipStreamSynchronize(st));
    return NT_OK;
  });
}

int nts_votes_sign(nt_ctx* ctx, const nts_signer* s, const uint8_t* id32, const uint64_t* round,
                   const uint8_t* origin32, uint64_t n, uint8_t* out_vote212, uint8_t* out_digest32) {
  if (!usable(ctx, s)) return NT_EINVAL;
  if (n == 0) return NT_OK;
  if (!id32 || !round || !origin32 || !out_vote212) return NT_EINVAL;
  if (small_verify(ctx, n, nt::kRouteKeyCache)) {
    nt::cpu::parallel_for(n, small_threads(ctx, n), [&](uint64_t i) {
      nt::cpu::vote(s->key, id32 + 32 * i, round[i], origin32 + 32 * i, out_vote212 + (uint64_t)NTS_VOTE_BYTES * i,
                    out_digest32 ? out_digest32 + 32 * i : nullptr);
    });
    ctx->calls_host++;
    return NT_OK;
  }
  ctx->calls_gpu++;
  // shards start at multiples of 64: every shard's output starts on a row boundary
  return run_sharded(ctx, n, 64, [&](Device& dv, uint64_t lo, uint64_t hi) -> int {
    NT_CHK(comb_b_for(dv));
    const uint64_t m = hi - lo;
    hipStream_t st = dv.lane[0].stream;
    NT_CHK(dv.d[B_DATA].ensure(m * 32));
    NT_CHK(dv.d[B_PK].ensure(m * 32));
    NT_CHK(dv.d[B_OFF].ensure(m * 8));
    NT_CHK(dv.d[B_OUT].ensure(m * NTS_VOTE_BYTES));
    if (out_digest32) NT_CHK(dv.d[B_OUT2].ensure(m * 32));
    NT_TRY(hipMemcpyAsync(dv.d[B_DATA].p, id32 + 32 * lo, m * 32, hipMemcpyHostToDevice, st));
    NT_TRY(hipMemcpyAsync(dv.d[B_OFF].p, round + lo, m * 8, hipMemcpyHostToDevice, st));
    NT_TRY(hipMemcpyAsync(dv.d[B_PK].p, origin32 + 32 * lo, m * 32, hipMemcpyHostToDevice, st));
    NT_TRY(nt::launch_signer_votes(s->d_key[dv.group], dv.d[B_DATA].as<uint8_t>(), dv.d[B_OFF].as<uint64_t>(),
                                   dv.d[B_PK].as<uint8_t>(), m, dv.d_combB, dv.bbits, dv.d[B_OUT].as<uint8_t>(),
                                   out_digest32 ? dv.d[B_OUT2].as<uint8_t>() : nullptr, dv.sign_blocks * 4, st));
    NT_TRY(hipMemcpyAsync(out_vote212 + (uint64_t)NTS_VOTE_BYTES * lo, dv.d[B_OUT].p, m * NTS_VOTE_BYTES,
                          hipMemcpyDeviceToHost, st));
    if (out_digest32)
      NT_TRY(hipMemcpyAsync(out_digest32 + 32 * lo, dv.d[B_OUT2].p, m * 32, hipMemcpyDeviceToHost, st));
    NT_TRY(hipStreamSynchronize(st));
    return NT_OK;
  });
}

int nts_dev_votes_sign(nt_ctx* ctx, const nts_signer* s, int dev, void* stream, const uint8_t* d_id32,
                       const uint64_t* d_round, const uint8_t* d_origin32, uint64_t n, uint8_t* d_vote212,
                       uint8_t* d_digest32) {
  Device* dv = dev_of(ctx, dev);
  if (!dv || !usable(ctx, s)) return NT_EINVAL;
  if (n == 0) return NT_OK;
  if (!d_id32 || !d_round || !d_origin32 || !d_vote212) return NT_EINVAL;
  const uintptr_t a16 = (uintptr_t)d_id32 | (uintptr_t)d_origin32 | (uintptr_t)d_vote212 | (uintptr_t)d_digest32;
  if ((a16 & 15u) || ((uintptr_t)d_round & 7u)) return NT_EINVAL;
  NT_TRY(hipSetDevice(dv->ordinal));
  std::lock_guard<std::mutex> lk(dv->mu);
  NT_CHK(comb_b_for(*dv));
  NT_TRY(nt::launch_signer_votes(s->d_key[dv->group], d_id32, d_round, d_origin32, n, dv->d_combB, dv->bbits, d_vote212,
                                 d_digest32, dv->sign_blocks * 4, (hipStream_t)stream));
  return NT_OK;
}

}  // extern "C"
