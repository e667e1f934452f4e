// msg_plan.hpp -- the layout walk of one bincode PrimaryMessage (bincode 1.x,
// fixint, little endian; host/wire.cpp): the pure integer part of the device
// parser (k_ingest.hip k_cert_parse), compiled for the device and for the host
// (tests/cpp/msgplan/ runs it under the sanitizers over mutated messages).
// Bytes are read through a loader functor -- ld.u32(off), ld.u64(off) -- and
// every count and offset is bounded by the message length before it is used:
// the walk reads nothing outside [0, len).
//
//   Header       u32 0 | u64 44 | author b64 (44) | u64 round | u64 np | np x (digest 32, worker u32) |
//                u64 nq | nq x digest 32 | id 32 | signature 64
//   Vote         u32 1 | id 32 | u64 round | u64 44 | origin b64 (44) | u64 44 | author b64 (44) |
//                signature 64                                                        (212 bytes)
//   Certificate  u32 2 | the header's body | u64 nv | nv x (u64 44 | key b64 (44) | signature 64)
//   Request      u32 3 | u64 nd | nd x digest 32 | u64 44 | requestor b64 (44)
// Bytes after a complete message are allowed (as in the host decoder).  A key
// string with a length prefix other than 44 cannot be a committee key's
// canonical text: such a message is left to the host decoder, like anything
// truncated, any tag above 3 and any count over the caps below.
#pragma once
#include <stdint.h>

#include "nt_common.hpp"

namespace nt {

constexpr uint32_t kMsgHeader = 0, kMsgVote = 1, kMsgCert = 2, kMsgRequest = 3;
constexpr uint32_t kMsgHost = 0xffu;  // MsgPlan::kind: the host decoder decides this message
// which kinds a call decides (bit k = tag k); the others come back as kMsgHost
constexpr uint32_t kMsgKindsCert = 1u << kMsgCert, kMsgKindsAll = 0xfu;
constexpr uint32_t kMsgMaxVotes = 1024;        // larger certificates go to the host decoder
constexpr uint64_t kMsgMaxEntries = 1u << 20;  // payload / parents / request entries (ditto)
constexpr uint64_t kMsgKeyChars = 44;          // base64 (padded) of 32 bytes
constexpr uint64_t kMsgVoteBytes = 212;

struct MsgPlan {
  uint32_t kind = kMsgHost;
  uint64_t round = 0;
  uint64_t np = 0, nq = 0, nv = 0;  // payload entries, parents, certificate votes
  uint64_t nd = 0;                  // a request's digests
  // byte offsets in the message: payload entries at 72; parents; the (claimed) id;
  // the message's own signature; a certificate's votes (116 bytes each)
  uint64_t off_par = 0, off_id = 0, off_sig = 0, off_votes = 0;
  // 44-character key strings (their length prefixes were checked): key0 = the
  // author of a header / certificate, a vote's origin, a request's requestor;
  // key1 = a vote's author
  uint64_t key0 = 0, key1 = 0;
};

template <class Ld>
NT_HD NT_INLINE MsgPlan msg_walk(const Ld& ld, uint64_t L, uint32_t kinds) {
  MsgPlan m, host;
  if (L < 4) return host;
  const uint32_t tag = ld.u32(0);
  if (tag > 3 || !((kinds >> tag) & 1u)) return host;
  if (tag == kMsgVote) {
    if (L < kMsgVoteBytes || ld.u64(44) != kMsgKeyChars || ld.u64(96) != kMsgKeyChars) return host;
    m.off_id = 4;
    m.round = ld.u64(36);
    m.key0 = 52;
    m.key1 = 104;
    m.off_sig = 148;
  } else if (tag == kMsgRequest) {
    if (L < 12 + 8 + kMsgKeyChars) return host;
    m.nd = ld.u64(4);
    if (m.nd > (L - 12) / 32 || m.nd > kMsgMaxEntries) return host;
    const uint64_t pos = 12 + 32 * m.nd;
    if (L - pos < 8 + kMsgKeyChars || ld.u64(pos) != kMsgKeyChars) return host;
    m.key0 = pos + 8;
  } else {
    if (L < 72 || ld.u64(4) != kMsgKeyChars) return host;
    m.key0 = 12;
    m.round = ld.u64(56);
    m.np = ld.u64(64);
    uint64_t pos = 72;
    if (m.np > (L - pos) / 36 || m.np > kMsgMaxEntries) return host;
    pos += 36 * m.np;
    if (L - pos < 8) return host;
    m.nq = ld.u64(pos);
    pos += 8;
    if (m.nq > (L - pos) / 32 || m.nq > kMsgMaxEntries) return host;
    m.off_par = pos;
    pos += 32 * m.nq;
    if (L - pos < 96 + (tag == kMsgCert ? 8u : 0u)) return host;
    m.off_id = pos;
    m.off_sig = pos + 32;
    pos += 96;
    if (tag == kMsgCert) {
      m.nv = ld.u64(pos);
      pos += 8;
      if (m.nv > (L - pos) / 116 || m.nv > kMsgMaxVotes) return host;
      m.off_votes = pos;
    }
  }
  m.kind = tag;
  return m;
}

// offset of the key string of certificate vote v < m.nv (its signature follows
// at + 44), 0 if its length prefix is not 44
template <class Ld>
NT_HD NT_INLINE uint64_t msg_cert_vote_key(const Ld& ld, const MsgPlan& m, uint64_t v) {
  const uint64_t q = m.off_votes + 116 * v;
  return ld.u64(q) == kMsgKeyChars ? q + 8 : 0;
}

}  // namespace nt
