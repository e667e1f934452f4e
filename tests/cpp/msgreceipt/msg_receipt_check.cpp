// TEST INFRASTRUCTURE: the receipt assembly of the device ingestion
// (narwhal-tusk_amd/csrc/msg_receipt.hpp over msg_plan.hpp's walk) on the host,
// a stand-alone program built with -fsanitize=address,undefined for
// tests/test_msg_receipt_host.py.
//
//   msg_receipt_check IN OUT
//
// IN (little endian): u32 n | u32 kinds | u64 gc_round, then per message
//   u32 len | u32 code | u32 author | u32 origin | digest slot i (32) |
//   digest slot n + i (32) | len wire bytes
// -- the code, the committee indices and the two SHA-512 outputs the device
// holds for the message when k_msg_receipt runs (the test takes them from its
// Python model).  OUT: n records of 128 bytes, assembled exactly as the kernel
// does: the walk, the id from the wire at off_id, the digest slot
// msg_receipt_digest_off names.  Every message is walked in a heap block of
// exactly its length behind a loader that aborts on a read outside it; a record
// whose offsets reach past the message, or whose words do not land in the C
// struct's fields (include/ntcrypto.h), aborts too.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../../include/ntcrypto.h"
#include "../../../narwhal-tusk_amd/csrc/msg_receipt.hpp"

namespace {

[[noreturn]] void die(const char* what, unsigned long long a = 0, unsigned long long b = 0) {
  fprintf(stderr, "msg_receipt_check: %s (%llu, %llu)\n", what, a, b);
  abort();
}

struct CheckedLd {
  const uint8_t* p;
  uint64_t n;
  void in(uint64_t o, uint64_t k) const {
    if (!(o <= n && n - o >= k)) die("read outside the message", o, n);
  }
  uint32_t u32(uint64_t o) const {
    uint32_t x;
    in(o, 4);
    memcpy(&x, p + o, 4);
    return x;
  }
  uint64_t u64(uint64_t o) const {
    uint64_t x;
    in(o, 8);
    memcpy(&x, p + o, 8);
    return x;
  }
};

std::vector<uint8_t> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) die("cannot open the input");
  std::vector<uint8_t> v;
  uint8_t buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

struct Reader {
  const std::vector<uint8_t>& v;
  size_t pos = 0;
  const uint8_t* take(size_t k) {
    if (v.size() - pos < k) die("truncated input", pos, k);
    const uint8_t* p = v.data() + pos;
    pos += k;
    return p;
  }
  uint32_t u32() {
    uint32_t x;
    memcpy(&x, take(4), 4);
    return x;
  }
  uint64_t u64() {
    uint64_t x;
    memcpy(&x, take(8), 8);
    return x;
  }
};

struct Msg {
  uint32_t len, code, author, origin;
  const uint8_t* wire;
};

// the record's extents lie inside the message
void check_extents(const nt_msg_receipt& r, uint64_t len) {
  const auto inside = [&](uint64_t o, uint64_t k) { return o <= len && len - o >= k; };
  if (r.kind == NT_RECEIPT_KIND_HOST) return;
  if (!inside(r.off_payload, 36ull * r.np) || !inside(r.off_parents, 32ull * r.nq) ||
      !inside(r.off_votes, 116ull * r.nv))
    die("a counted extent reaches past the message", r.kind, len);
  if (r.kind != 3 && (!inside(r.off_id, 32) || !inside(r.off_sig, 64))) die("id / signature past the message", r.kind, len);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) die("usage: msg_receipt_check IN OUT");
  const std::vector<uint8_t> in = slurp(argv[1]);
  Reader rd{in};
  const uint64_t n = rd.u32();
  const uint32_t kinds = rd.u32();
  const uint64_t gc_round = rd.u64();
  // the digests where the device keeps them: [claimed ids 32 n][SHA-512 outputs 64 n]
  std::vector<uint8_t> mbase(96 * n + 1, 0);
  std::vector<Msg> msgs;
  for (uint64_t i = 0; i < n; ++i) {
    Msg m;
    m.len = rd.u32();
    m.code = rd.u32();
    m.author = rd.u32();
    m.origin = rd.u32();
    memcpy(&mbase[32 * n + 32 * i], rd.take(32), 32);
    memcpy(&mbase[32 * n + 32 * (n + i)], rd.take(32), 32);
    m.wire = rd.take(m.len);
    msgs.push_back(m);
  }
  if (rd.pos != in.size()) die("bytes after the last message", rd.pos, in.size());
  FILE* out = fopen(argv[2], "wb");
  if (!out) die("cannot open the output");
  uint64_t decided = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const Msg& g = msgs[i];
    // a heap block of exactly the message's length: AddressSanitizer sees what the loader's check would miss
    uint8_t* blk = (uint8_t*)malloc(g.len ? g.len : 1);
    if (g.len) memcpy(blk, g.wire, g.len);
    const CheckedLd ld{blk, g.len};
    uint32_t w[nt::kReceiptWords];
    if (g.code == nt::kReceiptHostCode) {  // the device never walks these again
      nt::msg_receipt_words(nt::MsgPlan{}, g.code, 0, 0, gc_round, nullptr, nullptr, w);
    } else {
      const nt::MsgPlan m = nt::msg_walk(ld, g.len, kinds);
      if (m.kind == nt::kMsgHost) die("the walk leaves a message the model decided to the host", i, g.len);
      uint32_t id[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dig[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (m.kind != nt::kMsgRequest) {
        ld.in(m.off_id, 32);
        memcpy(id, blk + m.off_id, 32);
        const uint64_t o = nt::msg_receipt_digest_off(m.kind, n, i);
        if (o + 32 > 96 * n) die("digest slot outside the buffer", o, n);
        memcpy(dig, &mbase[o], 32);
      }
      nt::msg_receipt_words(m, g.code, g.author, g.origin, gc_round, id, dig, w);
      ++decided;
    }
    free(blk);
    nt_msg_receipt r;
    static_assert(sizeof r == 4 * nt::kReceiptWords, "the record is the 32 words");
    memcpy(&r, w, sizeof r);
    // the words land in the struct's fields
    const uint64_t round = w[6] | ((uint64_t)w[7] << 32);
    if (r.code != (w[0] & 0xffu) || r.kind != ((w[0] >> 8) & 0xffu) || r.flags != (w[0] >> 16) || r.author != w[1] ||
        r.origin != w[2] || r.np != w[3] || r.nq != w[4] || r.nv != w[5] || r.round != round ||
        r.off_payload != w[8] || r.off_parents != w[9] || r.off_id != w[10] || r.off_sig != w[11] ||
        r.off_votes != w[12] || memcmp(r.id, &w[13], 32) != 0 || memcmp(r.digest, &w[21], 32) != 0 ||
        memcmp(r.reserved, &w[29], 12) != 0)
      die("the words and the struct disagree", i);
    check_extents(r, g.len);
    if (fwrite(&r, sizeof r, 1, out) != 1) die("short write");
  }
  if (fclose(out) != 0) die("close failed");
  printf("msg_receipt_check: %llu records, %llu decided on the device\n", (unsigned long long)n,
         (unsigned long long)decided);
  return 0;
}
