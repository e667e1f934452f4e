// dev_api.cpp -- the device-resident entry points (nt_dev_*): enqueue-only calls on the
// caller's stream over the caller's device buffers.
#include "runtime.hpp"

using namespace ntrt;

// The key-cache launch of a device-API call on the caller's stream s.  The lanes' scratch is
// shared with the host entry points, each pair ordered against every other user by its event
// whatever the streams; successive device-API calls alternate between the lanes (like
// nt_dev_ed25519_verify's workspaces, on a counter of their own), so batches on two streams
// can overlap.
static int keyset_dev(Device& dv, const nt_keyset& ks, hipStream_t s, int mode, const uint32_t* d_key_idx,
                      const uint8_t* d_sig64, const uint8_t* d_msg, uint64_t msg_bytes, const uint64_t* d_off,
                      const uint64_t* d_len, uint64_t n, uint64_t* d_out_words, nt::KsGroups groups) {
  std::lock_guard<std::mutex> lk(dv.mu);
  NT_CHK(comb_b_for(dv));
  const nt::KsTabs tabs = ks_tabs(ks.t->dev[dv.group], ks.bits, ks.nkeys, dv);
  return dv.keyset_on(dv.lane[dv.ks_calls++ & 1], s, n, [&](nt::KsScratch scratch) {
    return nt::launch_verify_keyset(mode, tabs, scratch, d_key_idx, d_sig64, d_msg, msg_bytes, d_off, d_len, n,
                                    d_out_words, s, groups);
  });
}

extern "C" {

int nt_dev_stream(nt_ctx* ctx, int dev, int which, void** out) {
  if (!ctx || !out || dev < 0 || dev >= (int)ctx->devs.size() || (which != 0 && which != 1)) return NT_EINVAL;
  *out = (void*)ctx->devs[dev]->lane[which].stream;
  return NT_OK;
}

// ---- device-resident entry points ---------------------------------------
// `stream` is the caller's; NULL is HIP's NULL stream (not the library's), so a
// caller whose inputs come from work on the NULL stream is ordered after it.
int nt_dev_sha512_trunc32(nt_ctx* ctx, int dev, void* stream, const uint8_t* d_data, uint64_t data_bytes,
                          const uint64_t* d_off, const uint64_t* d_len, uint64_t n, uint32_t* d_bad,
                          uint8_t* d_out32) {
  Device* dv = dev_of(ctx, dev);
  if (!dv || (n && (!d_data || !d_off || !d_len || !d_out32))) return NT_EINVAL;
  NT_TRY(hipSetDevice(dv->ordinal));
  NT_TRY(nt::launch_sha512_trunc32(d_data, data_bytes, d_off, d_len, n, d_out32, (hipStream_t)stream, ~0ull, d_bad));
  return NT_OK;
}

int nt_dev_sha512_trunc32_bounded(nt_ctx* ctx, int dev, void* stream, const uint8_t* d_data, uint64_t data_bytes,
                                  const uint64_t* d_off, const uint64_t* d_len, uint64_t n, uint64_t max_len,
                                  uint32_t* d_bad, uint8_t* d_out32) {
  Device* dv = dev_of(ctx, dev);
  if (!dv || (n && (!d_data || !d_off || !d_len || !d_out32))) return NT_EINVAL;
  NT_TRY(hipSetDevice(dv->ordinal));
  NT_TRY(nt::launch_sha512_trunc32(d_data, data_bytes, d_off, d_len, n, d_out32, (hipStream_t)stream, max_len, d_bad));
  return NT_OK;
}

int nt_dev_ed25519_verify(nt_ctx* ctx, int dev, void* stream, int mode, const uint8_t* d_pk32,
                          const uint8_t* d_sig64, const uint8_t* d_msg, uint64_t msg_bytes, const uint64_t* d_off,
                          const uint64_t* d_len, uint64_t n, uint64_t* d_out_words) {
  Device* dv = dev_of(ctx, dev);
  if (!dv || (mode != NT_MODE_STRICT && mode != NT_MODE_COFACTORLESS)) return NT_EINVAL;
  if (n && (!d_pk32 || !d_sig64 || !d_msg || !d_off || !d_len || !d_out_words)) return NT_EINVAL;
  NT_TRY(hipSetDevice(dv->ordinal));
  // Successive calls alternate between the lanes' [k]A workspaces (each at its full ws_slots
  // slots), so back-to-back batches issued on two caller streams overlap -- the waves of the
  // next batch fill the SIMDs the previous batch's last round leaves idle.  Calls on one
  // stream stay in stream order.
  std::lock_guard<std::mutex> lk(dv->mu);
  NT_CHK(verify_tables(*dv));
  return dv->verify_on(dv->lane[dv->dev_calls++ & 1], (hipStream_t)stream, mode, d_pk32, d_sig64, d_msg, msg_bytes,
                       d_off, d_len, n, d_out_words, 0, dv->ws_slots);
}

int nt_dev_group_and(nt_ctx* ctx, int dev, void* stream, const uint64_t* d_first,
                     const uint32_t* d_cnt, uint64_t G, const uint64_t* d_sig_words,
                     uint64_t* d_group_words) {
  Device* dv = dev_of(ctx, dev);
  if (!dv) return NT_EINVAL;
  NT_TRY(hipSetDevice(dv->ordinal));
  NT_TRY(nt::launch_group_and(d_first, d_cnt, G, d_sig_words, d_group_words, (hipStream_t)stream));
  return NT_OK;
}

int nt_dev_ed25519_verify_keyset(nt_ctx* ctx, const nt_keyset* ks, int dev, void* stream, int mode,
                                 const uint32_t* d_key_idx, const uint8_t* d_sig64, const uint8_t* d_msg,
                                 uint64_t msg_bytes, const uint64_t* d_off, const uint64_t* d_len, uint64_t n,
                                 uint64_t* d_out_words) {
  Device* dv = dev_of(ctx, dev);
  if (!dv || !ks || ks->ctx != ctx || (mode != NT_MODE_STRICT && mode != NT_MODE_COFACTORLESS && mode != NT_MODE_MIXED))
    return NT_EINVAL;
  if (n && (!d_key_idx || !d_sig64 || !d_msg || !d_off || !d_len || !d_out_words)) return NT_EINVAL;
  NT_TRY(hipSetDevice(dv->ordinal));
  return keyset_dev(*dv, *ks, (hipStream_t)stream, mode, d_key_idx, d_sig64, d_msg, msg_bytes, d_off, d_len, n,
                    d_out_words, {});
}

int nt_dev_clock_probe(nt_ctx* ctx, int dev, void* stream, uint32_t iters, uint64_t* d_out2, uint64_t* wall_khz) {
  Device* dv = dev_of(ctx, dev);
  if (!dv || !d_out2 || iters == 0) return NT_EINVAL;
  NT_TRY(hipSetDevice(dv->ordinal));
  if (wall_khz) {
    int khz = 0;
    NT_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dv->ordinal));
    *wall_khz = (uint64_t)khz;
  }
  NT_TRY(nt::launch_clock_probe(iters, dv->real_cus, d_out2, (hipStream_t)stream));
  return NT_OK;
}

int nt_dev_ed25519_verify_keyset_groups(nt_ctx* ctx, const nt_keyset* ks, int dev, void* stream, int mode,
                                        const uint32_t* d_key_idx, const uint8_t* d_sig64, const uint8_t* d_msg,
                                        uint64_t msg_bytes, const uint64_t* d_off, const uint64_t* d_len, uint64_t n,
                                        const uint64_t* d_first, const uint32_t* d_cnt, uint64_t G,
                                        uint64_t* d_out_words, uint64_t* d_group_words) {
  Device* dv = dev_of(ctx, dev);
  if (!dv || !ks || ks->ctx != ctx || (mode != NT_MODE_STRICT && mode != NT_MODE_COFACTORLESS && mode != NT_MODE_MIXED))
    return NT_EINVAL;
  if (n && (!d_key_idx || !d_sig64 || !d_msg || !d_off || !d_len || !d_out_words)) return NT_EINVAL;
  if (G && (!d_first || !d_cnt || !d_group_words)) return NT_EINVAL;
  NT_TRY(hipSetDevice(dv->ordinal));
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return G ? (nt::launch_group_and(d_first, d_cnt, G, d_out_words, d_group_words, s) == hipSuccess
                              ? NT_OK : NT_EHIP)
                       : NT_OK;
  return keyset_dev(*dv, *ks, s, mode, d_key_idx, d_sig64, d_msg, msg_bytes, d_off, d_len, n, d_out_words,
                    nt::KsGroups{d_first, d_cnt, G, d_group_words});
}

int nt_dev_ed25519_sign(nt_ctx* ctx, int dev, void* stream, const uint8_t* d_seed32, const uint8_t* d_msg,
                        uint64_t msg_bytes, const uint64_t* d_off, const uint64_t* d_len, uint64_t n,
                        uint8_t* d_pk32, uint8_t* d_sig64) {
  Device* dv = dev_of(ctx, dev);
  if (!dv || (n && (!d_seed32 || !d_pk32))) return NT_EINVAL;
  if (n && d_sig64 && (!d_msg || !d_off || !d_len)) return NT_EINVAL;
  NT_TRY(hipSetDevice(dv->ordinal));
  std::lock_guard<std::mutex> lk(dv->mu);
  NT_CHK(comb_b_for(*dv));
  NT_TRY(nt::launch_sign(d_seed32, d_sig64 ? d_msg : nullptr, msg_bytes, d_off, d_len, n, dv->d_combB, dv->bbits,
                         d_pk32, d_sig64, dv->sign_blocks, (hipStream_t)stream));
  return NT_OK;
}

}  // extern "C"
