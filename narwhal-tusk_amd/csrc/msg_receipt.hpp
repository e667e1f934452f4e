// msg_receipt.hpp -- the 128-byte receipt of one ingested message
// (include/ntcrypto.h nt_msg_receipt) assembled from what the chunk holds when
// k_cert_verdict has run: the layout walk's plan (msg_plan.hpp), the committee
// indices of the key strings, the code, the id the message claims and the
// digest the SHA-512 launch computed.  Pure integer code, compiled for the
// device (k_ingest.hip k_msg_receipt) and for the host (tests/cpp/msgreceipt/
// runs it under the sanitizers and compares the records with a Python model).
//
// The record as 32 little-endian words (= eight 16-byte rows):
//   0  code | kind << 8 | flags << 16      8  off_payload     13..20  id
//   1  author                              9  off_parents     21..28  digest
//   2  origin                             10  off_id          29..31  zero
//   3  np   4  nq   5  nv                 11  off_sig
//   6, 7  round                           12  off_votes
#pragma once
#include <stdint.h>

#include "msg_plan.hpp"

namespace nt {

constexpr uint32_t kReceiptWords = 32;
constexpr uint32_t kReceiptHostCode = 0xffu;  // NT_DAG_HOST: kind 0xff, every other byte zero
constexpr uint32_t kReceiptGenesis = 1u;      // flags bit 0

// Where message i's digest lies in the chunk's mbase (CertBufs): the SHA-512
// launch writes output k at 32 n + 32 k; input i is a header's preimage or a
// vote's, input n + i a certificate's (k_cert_scatter).
NT_HD NT_INLINE uint64_t msg_receipt_digest_off(uint32_t kind, uint64_t n, uint64_t i) {
  return 32 * n + 32 * (kind == kMsgCert ? n + i : i);
}

// m: the plan of a message the device decided (m.kind != kMsgHost), or any plan
// when code is kReceiptHostCode.  author / origin: committee indices (a vote:
// key1 / key0; otherwise both key0's).  id: the 8 words at m.off_id, dig: the 8
// words at msg_receipt_digest_off -- neither is read for a request.  The genesis
// flag is k_cert_verdict's branch: a certificate of round 0 with a zero id that
// the round filter let through (gc_round == 0).
NT_HD NT_INLINE void msg_receipt_words(const MsgPlan& m, uint32_t code, uint32_t author, uint32_t origin,
                                       uint64_t gc_round, const uint32_t id[8], const uint32_t dig[8],
                                       uint32_t w[kReceiptWords]) {
#pragma unroll
  for (uint32_t k = 0; k < kReceiptWords; ++k) w[k] = 0;
  if (code == kReceiptHostCode || m.kind == kMsgHost) {
    w[0] = kReceiptHostCode | (kMsgHost << 8);
    return;
  }
  const bool req = m.kind == kMsgRequest;
  uint32_t idz = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) idz |= id[j];
  const bool genesis = m.kind == kMsgCert && m.round == 0 && gc_round == 0 && idz == 0;
  w[0] = (code & 0xffu) | (m.kind << 8) | ((genesis ? kReceiptGenesis : 0u) << 16);
  w[1] = author;
  w[2] = origin;
  w[3] = (uint32_t)m.np;
  w[4] = (uint32_t)(req ? m.nd : m.nq);
  w[5] = (uint32_t)m.nv;
  w[6] = (uint32_t)m.round;
  w[7] = (uint32_t)(m.round >> 32);
  w[8] = m.np ? 72u : 0u;
  w[9] = req ? 12u : (uint32_t)m.off_par;
  w[10] = (uint32_t)m.off_id;
  w[11] = (uint32_t)m.off_sig;
  w[12] = (uint32_t)m.off_votes;
  if (req) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    w[13 + j] = id[j];
    w[21 + j] = dig[j];
  }
}

}  // namespace nt
