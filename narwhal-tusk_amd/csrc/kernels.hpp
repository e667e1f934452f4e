// kernels.hpp -- host-side launchers of the k_*.hip kernels (used by the host runtime's units: verify.cpp, groups.cpp, sign.cpp, dev_api.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ks_plan.hpp"
#include "nt_common.hpp"

namespace nt {

// Every launcher that reads caller messages takes the byte size of the message
// buffer (msg_bytes / data_bytes): items whose slice lies outside it are never
// read (nt_common.hpp msg_slice) -- rejected by verification and signing, a
// zero digest counted in *d_bad (nullable) by SHA-512.
// max_len: an upper bound of the messages' lengths when the caller knows one
// (it selects the kernel; any length is still hashed correctly)
hipError_t launch_sha512_trunc32(const uint8_t* d_data, uint64_t data_bytes, const uint64_t* d_off,
                                 const uint64_t* d_len, uint64_t n, uint8_t* d_out32, hipStream_t s,
                                 uint64_t max_len = ~0ull, uint32_t* d_bad = nullptr);
// The x cache of a verify launch (kernels_common.hpp DevXCache): mask + 1 slots of 32 bytes
// (a power of two), tab == nullptr = no table.
struct XTab {
  void* tab = nullptr;
  uint32_t mask = 0;
};
// slot count of an x cache asked for as `want` slots: rounded down to a power of two, at most
// `cap` (a power of two); 0 = none
constexpr uint32_t kXCacheSlotsDefault = 1u << 21;  // 64 MB
constexpr uint32_t kXCacheSlotsMax = 1u << 28;      // 8 GB
inline uint32_t xcache_slots_pow2(unsigned long long want, uint32_t cap) {
  if (want == 0) return 0;
  uint32_t s = 1;
  while (s < cap && 2ull * s <= want) s <<= 1;
  return s;
}
// The key-table cache of a verify launch (kernels_common.hpp DevKTab; ktab.hpp):
// base = the control block (kKTabCtlBytes: words 0..3 = entries handed out, fast-path rows, builds,
// old-path rows; words 4..5 = the pool's device address, 128-byte aligned entries of
// ktab_entry_bytes(); word 6 = index slots - 1, a power of two of whole buckets; words 8..9 = the
// second pool's device address, ktab_ext_bytes() per entry index: the key's comb, or the fourth
// table of a -DNT_KCOMB=0 build) followed by
// the index slots of 8 bytes; cap = the pool entries this launch may use.  base == nullptr = none.
struct KTabArgs {
  void* base = nullptr;
  uint32_t cap = 0;
};
constexpr uint32_t kKTabCtlBytes = 128;
constexpr uint32_t kKTabKeysDefault = 1u << 20;   // 4.16 GB of entries + 4.43 GB of combs (8,192 B per key)
constexpr uint32_t kKTabKeysFloor = 1u << 14;     // the default halves down to this, then none
constexpr uint32_t kKTabIndexSlots = 1u << 21;    // 16 MB
constexpr uint32_t kKTabCtlWords = 4;
size_t ktab_entry_bytes();
size_t ktab_ext_bytes();
hipError_t launch_verify(int mode, const uint8_t* d_pk, const uint8_t* d_sig, const uint8_t* d_msg,
                         uint64_t msg_bytes, const uint64_t* d_off, const uint64_t* d_len, uint64_t n,
                         const uint32_t* d_combB, int bbits, void* d_ws, uint32_t ws_slots, uint64_t* d_out_words,
                         hipStream_t s, int per_lane = 0, XTab xt = XTab(), KTabArgs kt = KTabArgs());
hipError_t launch_group_and(const uint64_t* d_first, const uint32_t* d_cnt, uint64_t G,
                            const uint64_t* d_sig_words, uint64_t* d_group_words, hipStream_t s);
// off[first[g] + q] = 32 g, len = 32 for q < cnt[g] (groups' 32-byte messages)
hipError_t launch_group_msgs(const uint64_t* d_first, const uint32_t* d_cnt, uint64_t G, uint64_t* d_off,
                             uint64_t* d_len, hipStream_t s);
hipError_t launch_sign(const uint8_t* d_seed, const uint8_t* d_msg, uint64_t msg_bytes, const uint64_t* d_off,
                       const uint64_t* d_len, uint64_t n, const uint32_t* d_combB, int bbits, uint8_t* d_pk,
                       uint8_t* d_sig, uint32_t max_blocks, hipStream_t s);
// ---- the signer bound to one key (k_signer.hip, signer.cpp) ----
// d_key: the 192-byte key record (signer_ops.hpp SignerKey).  id / origin / digest / vote / sig
// arrays 16-byte aligned, round 8-byte aligned.  One vote per lane into vote[n][212] and, when
// d_digest is given, digest[n][32]; max_rows / max_blocks cap the grid (rows of 64 / blocks of 256).
hipError_t launch_signer_votes(const void* d_key, const uint8_t* d_id, const uint64_t* d_round, const uint8_t* d_origin,
                               uint64_t n, const uint32_t* d_combB, int bbits, uint8_t* d_vote, uint8_t* d_digest,
                               uint32_t max_rows, hipStream_t s);
hipError_t launch_signer_digests(const void* d_key, const uint8_t* d_digest, uint64_t n, const uint32_t* d_combB,
                                 int bbits, uint8_t* d_sig, uint32_t max_blocks, hipStream_t s);
// wide combs with `bits`-bit digits (a key-comb width, or kBCombBits for B; kBCombFallback = kKeyCombWide).
// bbits below: the digit width of the comb of B d_combB was built with (kBCombBits / kBCombFallback).
hipError_t launch_wcomb_build(int bits, const uint32_t* d_enc, uint32_t nkeys, int negate, uint32_t* d_comb,
                              uint32_t* d_meta, uint32_t* d_bases, uint32_t* d_tmp, uint32_t batch,
                              hipStream_t s);
// What a key-cache launch reads on one device: the combs of nkeys keys at key_bits-bit digits
// (meta: kKey* flags, enc: the encodings), the comb of B at bbits-bit digits, the device's CUs.
struct KsTabs {
  int key_bits;
  const uint32_t *meta, *enc, *combA;
  uint32_t nkeys;
  const uint32_t* combB;
  int bbits;
  uint32_t cus;
};
// Its scratch, both required: the per-wave stash (keyset_stash_bytes) and the chunk counter +
// key-grouped order (keyset_sort_bytes).  One launch at a time may use a pair.
struct KsScratch {
  void* stash;
  void* sort;
};
// Groups (optional, G > 0): the launch also ANDs the verdicts of each group of
// signatures [first[g], first[g] + cnt[g]) (first non-decreasing) into bit g of
// `words` -- inside the kernel's epilogue (KsVerdict, kernels_common.hpp), no
// k_group_and launch.
struct KsGroups {
  const uint64_t* first = nullptr;
  const uint32_t* cnt = nullptr;
  uint64_t G = 0;
  uint64_t* words = nullptr;
};
hipError_t launch_verify_keyset(int mode, const KsTabs& tabs, KsScratch scratch, const uint32_t* d_key_idx,
                                const uint8_t* d_sig, const uint8_t* d_msg, uint64_t msg_bytes, const uint64_t* d_off,
                                const uint64_t* d_len, uint64_t n, uint64_t* d_out_words, hipStream_t s,
                                KsGroups groups = {});
size_t keyset_sort_bytes(uint64_t n);
// the plan of one key-cache launch over n signatures on a device of `cus` CUs (ks_plan.hpp;
// NT_KEYSET_WAVES = 1 (streamed) / 2 / 3 forces the waves per SIMD, NT_KEYSET_PER_LANE caps the rows per chunk)
KsPlan keyset_plan(uint64_t n, uint32_t cus);
// signatures one full round of the launch covers (host-side chunk sizing)
uint64_t keyset_round_sigs(uint32_t cus);
// signatures per lane of a launch_verify: per_lane 0 = the build's default (kVPer, 2);
// 1 = one per lane (half the launch latency; host entry points' short chunks)
int verify_per_lane_for(int per_lane);
uint64_t verify_grid(uint64_t n, uint32_t ws_slots, int per_lane = 0);  // blocks of a launch_verify
uint64_t verify_round_sigs(uint32_t cus, int per_lane = 0);
uint32_t keyset_per_lane();
// per-wave stash of a launch over n signatures (d_stash above)
size_t keyset_stash_bytes(uint64_t n, uint32_t cus);
size_t wcomb_bytes_per_key(int bits);
size_t wcomb_bases_bytes_per_key(int bits);
size_t wcomb_fill_tmp_bytes_per_key(int bits);
uint32_t wcomb_fill_batch(int bits);  // keys per k_wcomb_fill launch
size_t ws_bytes_per_slot();
int verify_occupancy();  // waves per SIMD of the selected verify kernel variant
// diagnostics: d_out2[0] / d_out2[1] = summed shader-clock cycles / 100 MHz ticks of a fixed multiply load
hipError_t launch_clock_probe(uint32_t iters, uint32_t cus, uint64_t* d_out2, hipStream_t s);

// ---- certificate ingestion on the device (k_ingest.hip, ingest_gpu.cpp) ----
// Committee tables of an nt_committee on one device.
struct CertCommittee {
  const uint32_t* enc;        // [nkeys][12]: canonical base64 text of the key (44 chars) + 4 zero bytes
  const uint64_t* slot_head;  // [1 << sbits]: first 8 characters of the key in the slot
  const uint32_t* slot_idx;   // [1 << sbits]: key index, 0xffffffff = empty (open addressing)
  const uint32_t* stake;      // [nkeys]
  const uint32_t* wfirst;     // [nkeys + 1]: key k's workers are wids[wfirst[k] .. wfirst[k + 1]), sorted
  const uint32_t* wids;
  const uint32_t* raw;        // [nkeys][8]: the raw 32-byte keys (the keyset's encodings)
  uint32_t nkeys, sbits, quorum;
};
// One chunk of n messages: inputs, per-message state, launch buffers, outputs.
struct CertBufs {
  const uint8_t* wire;   // message bytes (64 bytes of readable slack on both sides)
  const uint64_t* moff;  // message i = wire[moff[i] .. moff[i] + mlen[i])
  const uint64_t* mlen;
  uint64_t n;
  uint32_t kinds;        // the kinds this call decides (msg_plan.hpp kMsgKinds*); the others come back "host"
  uint64_t* round;       // k_cert_parse
  uint32_t *author, *np, *nq, *nv, *flags, *plen;
  uint64_t *vbase, *pbase;  // k_cert_scan (n + 1 entries)
  uint8_t* mbase;        // [claimed ids 32 n][digests 64 n][certificate preimages 72 n][header preimages]
  uint64_t pre_off;      // offset of the header preimages in mbase
  uint32_t* keys;        // n + V key-cache launch entries: key index (| strict bit), signature, message
  uint4* sigs;
  uint64_t *smoff, *smlen;
  uint64_t *soff, *slen;   // 2 n SHA-512 inputs (offsets into mbase)
  uint64_t* gfirst;        // n vote groups
  uint32_t* gcnt;
  uint32_t *verr, *weight;
  const uint64_t* sig_words;  // verdict words of the key-cache launch
  const uint64_t* grp_words;  // group AND words
  uint8_t* code;              // per message: primary::DagError, 0xff = host decoder
  uint4* rec;                 // per message: the 128-byte receipt (msg_receipt.hpp); null = none asked for
};
hipError_t launch_cert_parse(const CertCommittee& c, const CertBufs& b, hipStream_t s);
hipError_t launch_cert_scan(const CertBufs& b, hipStream_t s);
hipError_t launch_cert_scatter(const CertCommittee& c, const CertBufs& b, hipStream_t s);
// The header currently being voted on (Core::current_header), as a vote's
// digest preimage spells it: id || round_le || author (18 words), and its round.
struct MsgCurrent {
  uint32_t w[18];
  uint64_t round;
};
hipError_t launch_cert_verdict(const CertCommittee& c, const CertBufs& b, uint64_t gc_round, const MsgCurrent& cur,
                               hipStream_t s);
// after launch_cert_verdict on the same stream; needs b.rec
hipError_t launch_msg_receipt(const CertCommittee& c, const CertBufs& b, uint64_t gc_round, hipStream_t s);

}  // namespace nt
