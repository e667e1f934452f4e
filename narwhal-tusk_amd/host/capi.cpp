// capi.cpp -- C entry points of libntnarwhal.so for the Python tests and bench.py
// (ctypes): the wire codec (CPU only) and the batched primary::Core ingestion
// path of SURVEY §8(f).1/(f).2 (GPU through libntcrypto).  Not part of the
// crypto crate's boundary (include/ntcrypto.h is).
#include <algorithm>
#include <cstring>
#include <future>
#include <exception>
#include <memory>

#include "../../include/ntcrypto.h"
#include "narwhal.hpp"
#include "wire.hpp"

namespace {
struct CoreHandle {
  primary::Committee committee;
  std::unique_ptr<crypto::KeySet> keyset;
  std::unique_ptr<primary::VoteSigner> signer;
  primary::Core core;
};
}  // namespace

extern "C" {

// Decode one bincode PrimaryMessage and encode it again.  Returns the encoded
// length (<= cap written to out), -1 on a decode error, -2 if cap is too small.
// `used` receives the number of input bytes the decoder consumed.
int64_t ntn_wire_reencode(const uint8_t* data, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* used) {
  primary::PrimaryMessage m;
  size_t u = 0;
  if (!primary::decode(data, (size_t)len, m, &u)) return -1;
  if (used) *used = u;
  const auto v = primary::encode(m);
  if (v.size() > cap) return -2;
  std::memcpy(out, v.data(), v.size());
  return (int64_t)v.size();
}

// Header digest (messages.rs:70-84) of a decoded bincode PrimaryMessage::Header
// or ::Certificate, computed on the host preimage (CPU check of the layout);
// returns the preimage length or -1.
int64_t ntn_wire_header_preimage(const uint8_t* data, uint64_t len, uint8_t* out, uint64_t cap) {
  primary::PrimaryMessage m;
  if (!primary::decode(data, (size_t)len, m)) return -1;
  const primary::Header& h = m.kind == primary::MsgKind::Certificate ? m.certificate.header : m.header;
  const auto v = h.digest_preimage();
  if (v.size() > cap) return -2;
  std::memcpy(out, v.data(), v.size());
  return (int64_t)v.size();
}

// Committee of n authorities (keys32[n][32], stake[n], workers 0..nworkers[i]-1),
// Core state (gc_round, current header as bincode of a PrimaryMessage::Header,
// may be null), optional committee key cache.  Returns null on failure.
void* ntn_core_new(const uint8_t* keys32, const uint32_t* stakes, const uint32_t* nworkers, uint32_t n,
                   uint64_t gc_round, const uint8_t* cur_header, uint64_t cur_len, int use_keyset) {
  try {
    auto h = std::make_unique<CoreHandle>();
    for (uint32_t i = 0; i < n; ++i) {
      crypto::PublicKey pk;
      std::memcpy(pk.bytes.data(), keys32 + 32 * (size_t)i, 32);
      primary::Authority a;
      a.stake = stakes[i];
      for (uint32_t w = 0; w < nworkers[i]; ++w) a.workers.insert(w);
      h->committee.authorities[pk] = a;
    }
    if (cur_header) {
      primary::PrimaryMessage m;
      if (!primary::decode(cur_header, (size_t)cur_len, m) || m.kind != primary::MsgKind::Header) return nullptr;
      h->core.current_header = m.header;
    }
    if (use_keyset) h->keyset = primary::committee_keyset(h->committee);
    h->core.committee = &h->committee;
    h->core.gc_round = gc_round;
    h->core.cache = h->keyset.get();
    return h.release();
  } catch (const std::exception&) {
    return nullptr;
  }
}

void ntn_core_free(void* p) { delete (CoreHandle*)p; }

// Core::ingest over n packed wire messages: out_codes[i] = primary::DagError.
// Returns 0, or -2 on a backend failure (never reported as a verdict).
// general = 1: the object-model decoder + sanitize_batch (cross-check path);
// general = 2: Core::ingest_device (certificates parsed on the GPU), and
// decode_seconds then returns the count of messages left to the host decoder;
// general = 3: Core::ingest_device_all (every kind decided on the GPU), same return.
int ntn_core_ingest(void* p, const uint8_t* data, const uint64_t* off, const uint64_t* len, uint64_t n,
                    int threads, int32_t* out_codes, double* decode_seconds, int general) {
  try {
    const auto& core = ((CoreHandle*)p)->core;
    std::vector<primary::DagError> r;
    if (general == 2 || general == 3) {
      size_t host = 0;
      r = general == 3 ? core.ingest_device_all(data, off, len, (size_t)n, threads, &host)
                       : core.ingest_device(data, off, len, (size_t)n, threads, &host);
      if (decode_seconds) *decode_seconds = (double)host;  // modes 2, 3: messages left to the host decoder
    } else {
      r = general ? core.ingest_general(data, off, len, (size_t)n, threads, decode_seconds)
                  : core.ingest(data, off, len, (size_t)n, threads, decode_seconds);
    }
    for (uint64_t i = 0; i < n; ++i) out_codes[i] = (int32_t)r[i];
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}

// Core::ingest_device_receipts: ingest mode 3's codes plus n 128-byte receipts
// (nt_msg_receipt) in out_receipts; *host_decided = messages left to the host decoder.
int ntn_core_ingest_receipts(void* p, const uint8_t* data, const uint64_t* off, const uint64_t* len, uint64_t n,
                             int threads, int32_t* out_codes, uint8_t* out_receipts, uint64_t* host_decided) {
  try {
    size_t host = 0;
    const auto r = ((CoreHandle*)p)->core.ingest_device_receipts(data, off, len, (size_t)n,
                                                                 (nt_msg_receipt*)out_receipts, threads, &host);
    for (uint64_t i = 0; i < n; ++i) out_codes[i] = (int32_t)r[i];
    if (host_decided) *host_decided = host;
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}

// The node's own key of a Core (seed32; null removes it): name32 (nullable) gets the public key.
int ntn_core_set_signer(void* p, const uint8_t* seed32, uint8_t* name32) {
  try {
    auto* h = (CoreHandle*)p;
    h->core.signer = nullptr;
    h->signer.reset();
    if (!seed32) return 0;
    h->signer = std::make_unique<primary::VoteSigner>(seed32);
    h->core.signer = h->signer.get();
    if (name32) std::memcpy(name32, h->signer->name().bytes.data(), 32);
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}

// Core::votes_for: out_votes212 gets m x 212 wire bytes for the headers receipts[selected[k]].
// Returns 0, -1 for a selected receipt that is no header's, -2 on a backend failure (no signer).
int ntn_core_votes_for(void* p, const uint8_t* receipts, const uint32_t* selected, uint64_t m, uint8_t* out_votes212) {
  try {
    const auto v = ((CoreHandle*)p)->core.votes_for((const nt_msg_receipt*)receipts, selected, (size_t)m);
    if (!v.empty()) std::memcpy(out_votes212, v.data(), v.size());
    return 0;
  } catch (const std::invalid_argument&) {
    return -1;
  } catch (const std::exception&) {
    return -2;
  }
}

// Core::ingest_pipelined: chunks of `chunk` messages, two in flight.
int ntn_core_ingest_pipelined(void* p, const uint8_t* data, const uint64_t* off, const uint64_t* len, uint64_t n,
                              int threads, uint64_t chunk, int32_t* out_codes) {
  try {
    const auto r = ((CoreHandle*)p)->core.ingest_pipelined(data, off, len, (size_t)n, threads, (size_t)chunk);
    for (uint64_t i = 0; i < n; ++i) out_codes[i] = (int32_t)r[i];
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}

// phase times of the calling thread's last ingest: decode, prep, digest,
// verify_strict, verify_batch, total (seconds)
void ntn_last_ingest_stats(double out[6]) {
  const auto& s = primary::last_ingest_stats();
  out[0] = s.decode;
  out[1] = s.prep;
  out[2] = s.digest;
  out[3] = s.strict;
  out[4] = s.batch;
  out[5] = s.total;
}

// ---- worker::DigestBatcher -------------------------------
void* ntn_batcher_new(uint64_t max_bytes, uint64_t max_batches, uint32_t max_delay_us) {
  try {
    worker::DigestBatcher::Policy p;
    p.max_bytes = (size_t)max_bytes;
    p.max_batches = (size_t)max_batches;
    p.max_delay_us = max_delay_us;
    return new worker::DigestBatcher(p);
  } catch (const std::exception&) {
    return nullptr;
  }
}
void ntn_batcher_free(void* b) { delete (worker::DigestBatcher*)b; }

// queue one serialized batch of Processor (worker_id, own); returns a ticket
// for ntn_batcher_wait (NULL on failure)
void* ntn_batcher_submit(void* b, uint32_t worker_id, int own, const uint8_t* data, uint64_t len) {
  try {
    worker::Processor p{worker_id, own != 0};
    return new std::future<worker::DigestBatcher::Output>(
        ((worker::DigestBatcher*)b)->submit(p, data, (size_t)len));
  } catch (const std::exception&) {
    return nullptr;
  }
}

// wait for a ticket (and free it): digest32 (32 bytes) and the Processor's
// 40-byte output message; 0, or -2 if the backend failed
int ntn_batcher_wait(void* ticket, uint8_t* digest32, uint8_t* msg40) {
  auto* f = (std::future<worker::DigestBatcher::Output>*)ticket;
  int rc = 0;
  try {
    const auto o = f->get();
    std::memcpy(digest32, o.digest.bytes.data(), 32);
    std::memcpy(msg40, o.message.data(), std::min<size_t>(40, o.message.size()));
  } catch (const std::exception&) {
    rc = -2;
  }
  delete f;
  return rc;
}

void ntn_batcher_flush(void* b) { ((worker::DigestBatcher*)b)->flush(); }

// flushes, batches, bytes, seconds inside nt_sha512_trunc32
void ntn_batcher_stats(void* b, double out[4]) {
  const auto s = ((worker::DigestBatcher*)b)->stats();
  out[0] = (double)s.flushes;
  out[1] = (double)s.batches;
  out[2] = (double)s.bytes;
  out[3] = s.hash_seconds;
}

// ---- the worker's drain ----------------------------------------------------
// worker::decode_message, the plain host decoder: the kind (0 batch, 1 request) or -1 on a
// bincode error; out3 = count (transactions / digests), bytes consumed, sum of the
// transaction lengths; key32 = a request's requestor.
int ntn_worker_decode(const uint8_t* data, uint64_t len, uint64_t* out3, uint8_t* key32) {
  try {
    worker::WorkerMessage m;
    size_t used = 0;
    if (!worker::decode_message(data, (size_t)len, m, &used)) return -1;
    const bool batch = m.kind == worker::WorkerMessage::Kind::Batch;
    uint64_t bytes = 0;
    for (const auto& tx : m.batch) bytes += tx.size();
    out3[0] = batch ? m.batch.size() : m.digests.size();
    out3[1] = used;
    out3[2] = bytes;
    if (!batch) std::memcpy(key32, m.requestor.bytes.data(), 32);
    return batch ? 0 : 1;
  } catch (const std::exception&) {
    return -1;
  }
}

// worker::ingest_device over n packed wire messages.  Per message: out_codes (NT_WMSG_OK /
// NT_WMSG_SERIALIZATION), out_kinds (0 batch, 1 request; 0xff when the code is not OK),
// out_msg40 (a batch: the Processor's 40-byte OthersBatch(digest, worker_id); else zero),
// out_key32 (a request's requestor; else zero), out_nd (a request's digests), and
// out_receipts, the n 64-byte records (nt_worker_receipt) as the device wrote them.
// Returns 0, or -2 on a backend failure.
int ntn_worker_ingest(uint32_t worker_id, const uint8_t* data, const uint64_t* off, const uint64_t* len, uint64_t n,
                      uint8_t* out_codes, uint8_t* out_kinds, uint8_t* out_msg40, uint8_t* out_key32,
                      uint32_t* out_nd, uint8_t* out_receipts, uint64_t* host_decided) {
  try {
    size_t host = 0;
    const auto r = worker::ingest_device(worker_id, data, off, len, (size_t)n, (nt_worker_receipt*)out_receipts, &host);
    std::memset(out_msg40, 0, 40 * (size_t)n);
    std::memset(out_key32, 0, 32 * (size_t)n);
    for (uint64_t i = 0; i < n; ++i) {
      out_codes[i] = r[i].code;
      out_kinds[i] = r[i].code == NT_WMSG_OK ? (uint8_t)r[i].kind : (uint8_t)NT_WORKER_KIND_NONE;
      out_nd[i] = (uint32_t)r[i].digests.size();
      if (r[i].code != NT_WMSG_OK) continue;
      if (r[i].kind == worker::WorkerMessage::Kind::Batch)
        std::memcpy(out_msg40 + 40 * i, r[i].message.data(), std::min<size_t>(40, r[i].message.size()));
      else
        std::memcpy(out_key32 + 32 * i, r[i].requestor.bytes.data(), 32);
    }
    if (host_decided) *host_decided = host;
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}

// the small-call path of the mirror's shared context (include/ntcrypto.h)
int ntn_set_small_call_path(int mode, int threads) {
  try {
    return nt_set_small_call_path(crypto::Backend::global().ctx(), mode, threads);
  } catch (const std::exception&) {
    return -2;
  }
}

}  // extern "C"
