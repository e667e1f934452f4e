// sign.cpp -- digests, signing and key generation: nt_sha512_trunc32,
// nt_ed25519_sign_batch, nt_ed25519_keypair_batch.
#include "pipeline.hpp"

using namespace ntrt;

namespace {

// Stage the message span used by items [lo, hi) (rebased offsets, 16-B phase kept).
int stage_messages(Device& dv, const uint8_t* data, const uint64_t* off, const uint64_t* len,
                   uint64_t lo, uint64_t hi, uint64_t* base_out, uint64_t* span_out) {
  uint64_t mn = UINT64_MAX, mx = 0;
  for (uint64_t i = lo; i < hi; ++i) {
    if (len[i] == 0) continue;
    mn = std::min(mn, off[i]);
    mx = std::max(mx, off[i] + len[i]);
  }
  if (mn == UINT64_MAX) mn = mx = 0;
  const uint64_t base = mn & ~(uint64_t)15;
  const uint64_t span = mx - base;
  const uint64_t m = hi - lo;
  NT_CHK(dv.d[B_DATA].ensure(span + 64));
  NT_CHK(dv.d[B_OFF].ensure(m * 8));
  NT_CHK(dv.d[B_LEN].ensure(m * 8));
  NT_CHK(dv.h[B_OFF].ensure(m * 8));
  NT_CHK(dv.h[B_LEN].ensure(m * 8));
  uint64_t* ho = dv.h[B_OFF].as<uint64_t>();
  uint64_t* hl = dv.h[B_LEN].as<uint64_t>();
  for (uint64_t i = lo; i < hi; ++i) {
    ho[i - lo] = len[i] ? off[i] - base : 0;
    hl[i - lo] = len[i];
  }
  if (span) NT_TRY(hipMemcpyAsync(dv.d[B_DATA].p, data + base, span, hipMemcpyHostToDevice, dv.lane[0].stream));
  NT_TRY(hipMemcpyAsync(dv.d[B_OFF].p, ho, m * 8, hipMemcpyHostToDevice, dv.lane[0].stream));
  NT_TRY(hipMemcpyAsync(dv.d[B_LEN].p, hl, m * 8, hipMemcpyHostToDevice, dv.lane[0].stream));
  *base_out = base;
  *span_out = span;
  return NT_OK;
}

}  // namespace

extern "C" {

int nt_sha512_trunc32(nt_ctx* ctx, const uint8_t* data, const uint64_t* off, const uint64_t* len,
                      uint64_t n, uint8_t* out32) {
  if (!ctx || (n && (!off || !len || !out32))) return NT_EINVAL;
  if (n == 0) return NT_OK;
  if (small_sha(ctx, n, len)) {
    nt::cpu::parallel_for(n, small_threads(ctx, n), [&](uint64_t i) {
      nt::cpu::sha512_trunc32(data + off[i], len[i], out32 + 32 * i);
    });
    ctx->calls_host++;
    return NT_OK;
  }
  ctx->calls_gpu++;
  return run_sharded(ctx, n, 64, [&](Device& dv, uint64_t lo, uint64_t hi) -> int {
    const uint64_t m = hi - lo;
    // a launch's time is set by its longest message: chunks of >= 64k messages
    const Chunks ch = nt::plan_chunks(chunk_targets(m, pipe_round(1 << 16)));
    MsgStage ms;
    NT_CHK(msg_prepare(dv, off, len, lo, ch, ms));
    NT_CHK(dv.d[B_OUT].ensure(m * 32));
    NT_CHK(run_chunks(dv, ch.size(), ms_pinned(ms, data), [&](size_t c) -> int {
      return msg_copy(dv, data, off, len, lo, ms, c, ch[c].first, ch[c].second);
    }, [&](size_t c) -> int {
      const uint64_t a = ch[c].first, b = ch[c].second;
      uint64_t ml = 0;  // the chunk's longest message selects the kernel
      for (uint64_t i = lo + a; i < lo + b; ++i) ml = std::max(ml, len[i]);
      NT_TRY(nt::launch_sha512_trunc32(dv.d[B_DATA].as<uint8_t>(), ms.span, chunk_off(dv, a),
                                       chunk_len(dv, a, b), b - a, dv.d[B_OUT].as<uint8_t>() + 32 * a,
                                       dv.cstr((int)c), ml));
      return NT_OK;
    }));
    NT_CHK(finish_chunks(dv));
    NT_TRY(hipMemcpyAsync(out32 + 32 * lo, dv.d[B_OUT].p, m * 32, hipMemcpyDeviceToHost, dv.lane[0].stream));
    NT_TRY(hipStreamSynchronize(dv.lane[0].stream));
    return NT_OK;
  }, sha_latency(n, len));
}

int nt_ed25519_sign_batch(nt_ctx* ctx, const uint8_t* seed32, const uint8_t* msg,
                          const uint64_t* off, const uint64_t* len, uint64_t n, uint8_t* pk32,
                          uint8_t* sig64) {
  if (!ctx || (n && (!seed32 || !pk32))) return NT_EINVAL;
  if (sig64 && n && (!off || !len)) return NT_EINVAL;
  if (n == 0) return NT_OK;
  return run_sharded(ctx, n, 64, [&](Device& dv, uint64_t lo, uint64_t hi) -> int {
    NT_CHK(comb_b_for(dv));
    const uint64_t m = hi - lo;
    const uint8_t* d_msg = nullptr;
    const uint64_t *d_off = nullptr, *d_len = nullptr;
    uint64_t span = 0;
    if (sig64) {
      uint64_t base;
      NT_CHK(stage_messages(dv, msg, off, len, lo, hi, &base, &span));
      d_msg = dv.d[B_DATA].as<uint8_t>();
      d_off = dv.d[B_OFF].as<uint64_t>();
      d_len = dv.d[B_LEN].as<uint64_t>();
    }
    NT_CHK(dv.d[B_PK].ensure(m * 32));
    NT_CHK(dv.d[B_SIG].ensure(m * 64));
    NT_CHK(dv.d[B_OUT].ensure(m * 32));
    NT_TRY(hipMemcpyAsync(dv.d[B_OUT].p, seed32 + 32 * lo, m * 32, hipMemcpyHostToDevice, dv.lane[0].stream));
    NT_TRY(nt::launch_sign(dv.d[B_OUT].as<uint8_t>(), d_msg, span, d_off, d_len, m, dv.d_combB, dv.bbits,
                           dv.d[B_PK].as<uint8_t>(), sig64 ? dv.d[B_SIG].as<uint8_t>() : nullptr,
                           dv.sign_blocks, dv.lane[0].stream));
    NT_TRY(hipMemcpyAsync(pk32 + 32 * lo, dv.d[B_PK].p, m * 32, hipMemcpyDeviceToHost, dv.lane[0].stream));
    if (sig64)
      NT_TRY(hipMemcpyAsync(sig64 + 64 * lo, dv.d[B_SIG].p, m * 64, hipMemcpyDeviceToHost, dv.lane[0].stream));
    NT_TRY(hipStreamSynchronize(dv.lane[0].stream));
    return NT_OK;
  });
}

int nt_ed25519_keypair_batch(nt_ctx* ctx, const uint8_t* seed32, uint64_t n, uint8_t* pk32) {
  return nt_ed25519_sign_batch(ctx, seed32, nullptr, nullptr, nullptr, n, pk32, nullptr);
}

}  // extern "C"
