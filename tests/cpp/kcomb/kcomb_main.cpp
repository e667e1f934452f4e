// kcomb_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program (built with
// -fsanitize=address,undefined) that runs ktab_build with a comb pool + verify_kc over a corpus
// file on the host policy and checks the labels.  File: u32 n, then per entry pk[32] sig[64]
// strict u8, batch_rule u8, u32 len, msg[len].  Exit 0 = every verdict is its label.
#include <cstdio>
#include <vector>

#include "kc_common.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n = 0, bad = 0;
  if (std::fread(&n, 4, 1, f) != 1) return 2;
  for (uint32_t i = 0; i < n; ++i) {
    uint8_t pk[32], sig[64], label[2];
    uint32_t len = 0;
    if (std::fread(pk, 32, 1, f) != 1 || std::fread(sig, 64, 1, f) != 1 || std::fread(label, 2, 1, f) != 1 ||
        std::fread(&len, 4, 1, f) != 1)
      return 2;
    // whole 4-byte granules (sha512.hpp reads the aligned granules that hold message bytes), and
    // never a null pointer, also for an empty message
    std::vector<uint8_t> msg(((size_t)len + 4) & ~(size_t)3);
    if (len && std::fread(msg.data(), len, 1, f) != 1) return 2;
    for (int mode = 0; mode < 2; ++mode) {
      const int got = kc::verify(mode, pk, sig, msg.data(), len);
      if (got != (int)label[mode]) {
        std::printf("entry %u mode %d: got %d, label %d\n", i, mode, got, (int)label[mode]);
        ++bad;
      }
    }
  }
  std::fclose(f);
  std::printf("%u entries x 2 modes, %u wrong\n", n, bad);
  return bad ? 1 : 0;
}
