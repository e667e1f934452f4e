// TEST INFRASTRUCTURE: the signer's per-lane operations (narwhal-tusk_amd/csrc/signer_ops.hpp)
// on the host, over a 12-bit host comb of B built the way the host lane builds its own.  A
// stand-alone program under the address and undefined-behaviour sanitizers for
// tests/test_signer_host.py: it reads seeds, votes, digests, (seed, message) pairs and keys
// from a file and writes what signer_key_setup, vote_digest_words, sign_fixed_one,
// vote_wire_words, sign_one and b64_encode32 make of them.  The vote records are written in
// place into a heap buffer of exactly n x 212 bytes, so an overrun is caught.
//
//   in : u32 nsigner, nvote, ndigest, npair, nkey
//        nsigner x seed[32]
//        nvote   x { u32 signer, id[32], u64 round, origin[32] }
//        ndigest x { u32 signer, digest[32] }
//        npair   x { seed[32], msg[32] }
//        nkey    x key[32]
//   out: nsigner x { A[32], text[44] }
//        nvote x vote[212], nvote x digest[32]
//        ndigest x sig[64]
//        npair x { sign_fixed_one sig[64], sign_one sig[64], sign_one A[32] }
//        nkey x text[44]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../narwhal-tusk_amd/csrc/signer_ops.hpp"

using namespace nt;

namespace {

constexpr int kBits = 12;
using HG = CombGeom<kBits>;

struct HostComb {
  static constexpr int kBits = ::kBits;
  const uint32_t* base;
  void load(uint32_t pos, uint32_t idx, ge_niels& q) const {
    const uint32_t* e = base + ((size_t)pos * HG::kEntries + idx) * kWStride;
    for (int i = 0; i < 10; ++i) {
      q.ypx.v[i] = e[i];
      q.ymx.v[i] = e[10 + i];
      q.xy2d.v[i] = e[20 + i];
    }
  }
};

std::vector<uint32_t> build_comb() {
  std::vector<uint32_t> comb(HG::kWordsPerPoint, 0u);
  uint32_t enc[8];
  for (int i = 0; i < 8; ++i) enc[i] = kBaseEnc[i];
  ge_p3 B;
  ge_frombytes_w(B, enc);
  std::vector<uint32_t> bases((size_t)HG::kPos * 40);
  wcomb_bases<kBits>(bases.data(), B);
  for (uint32_t pos = 0; pos < (uint32_t)HG::kPos; ++pos)
    for (uint32_t c = 0; c < (uint32_t)HG::kChunks; ++c) {
      uint32_t tmp[kWChunk * 10];
      uint32_t* dst = comb.data() + ((size_t)pos * HG::kEntries + 1 + (size_t)kWChunk * c) * kWStride;
      wcomb_fill<kBits>(dst, tmp, bases.data() + (size_t)pos * 40, c);
    }
  return comb;
}

struct Reader {
  const std::vector<uint8_t>& b;
  size_t at = 0;
  void take(void* dst, size_t n) {
    if (at + n > b.size()) {
      std::fprintf(stderr, "input truncated at %zu\n", at);
      std::exit(2);
    }
    std::memcpy(dst, b.data() + at, n);
    at += n;
  }
  uint32_t u32() {
    uint32_t v;
    take(&v, 4);
    return v;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: signer_check <in> <out>\n");
    return 2;
  }
  std::vector<uint8_t> in;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
  }
  Reader rd{in};
  const uint32_t nsigner = rd.u32(), nvote = rd.u32(), ndigest = rd.u32(), npair = rd.u32(), nkey = rd.u32();
  const std::vector<uint32_t> comb = build_comb();
  const HostComb wb{comb.data()};
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;

  std::vector<SignerKey> keys(nsigner);
  for (uint32_t i = 0; i < nsigner; ++i) {
    uint32_t sw[8];
    rd.take(sw, 32);
    signer_key_setup(keys[i], sw, wb);
    std::fwrite(keys[i].A, 1, 32, out);
    std::fwrite(keys[i].text, 1, 44, out);
  }

  // exactly nvote x 212 bytes, written in place (malloc: 16-byte aligned, records 4-byte aligned)
  uint8_t* votes = (uint8_t*)std::malloc((size_t)nvote * kVoteWireBytes + (nvote ? 0 : 1));
  std::vector<uint32_t> digests((size_t)nvote * 8);
  for (uint32_t i = 0; i < nvote; ++i) {
    const uint32_t k = rd.u32();
    uint32_t id[8], origin[8];
    uint64_t round;
    rd.take(id, 32);
    rd.take(&round, 8);
    rd.take(origin, 32);
    if (k >= nsigner) return 2;
    uint32_t* dg = digests.data() + 8 * (size_t)i;
    vote_digest_words(dg, id, round, origin);
    uint32_t Rw[8], s[8];
    sign_fixed_one(Rw, s, keys[k], dg, wb);
    vote_wire_words((uint32_t*)(votes + (size_t)kVoteWireBytes * i), id, round, origin, keys[k].text, Rw, s);
  }
  if (nvote) {
    std::fwrite(votes, 1, (size_t)nvote * kVoteWireBytes, out);
    std::fwrite(digests.data(), 4, digests.size(), out);
  }
  std::free(votes);

  for (uint32_t i = 0; i < ndigest; ++i) {
    const uint32_t k = rd.u32();
    uint32_t m[8], sig[16];
    rd.take(m, 32);
    if (k >= nsigner) return 2;
    sign_fixed_one(sig, sig + 8, keys[k], m, wb);
    std::fwrite(sig, 4, 16, out);
  }

  uint32_t differ = 0;
  for (uint32_t i = 0; i < npair; ++i) {
    uint32_t sw[8], m[8];
    rd.take(sw, 32);
    rd.take(m, 32);
    SignerKey key;
    signer_key_setup(key, sw, wb);
    uint32_t fixed[16], ref[16], A[8];
    sign_fixed_one(fixed, fixed + 8, key, m, wb);
    uint8_t msg[32];
    std::memcpy(msg, m, 32);
    sign_one(A, ref, ref + 8, sw, msg, 32, wb);
    differ += std::memcmp(fixed, ref, 64) != 0 || std::memcmp(A, key.A, 32) != 0;
    std::fwrite(fixed, 4, 16, out);
    std::fwrite(ref, 4, 16, out);
    std::fwrite(A, 4, 8, out);
  }

  for (uint32_t i = 0; i < nkey; ++i) {
    uint32_t k[8], text[11];
    rd.take(k, 32);
    b64_encode32(text, k);
    std::fwrite(text, 4, 11, out);
  }
  std::fclose(out);
  std::printf("%u signers %u votes %u digests %u pairs (%u differ) %u keys\n", nsigner, nvote, ndigest, npair, differ,
              nkey);
  return differ ? 1 : 0;
}
