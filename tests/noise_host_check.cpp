// Host check of the product's bit-sliced noise (csrc/cvd_common.h noise_word, the form the host
// learning chain and the generic generator kernel use): reads lines
//   seed tag seq_id w thr valid      (decimal; thr in [0, 2^32])
// from standard input and prints noise_word's flip mask of each, one hex word per line.
// tests/test_noise_host.py compiles it with g++ and compares the masks with the numpy spec
// (oracle/philox.py: (u < thr) & valid).  TEST INFRASTRUCTURE ONLY.
#include <cinttypes>
#include <cstdio>

#include "../detecting-convolutional-codes-via-markovian-statistics_amd/csrc/cvd_common.h"

using namespace cvd;

int main() {
  uint64_t seed, tag, seq_id, w, thr, valid;
  int lines = 0;
  while (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &seed, &tag, &seq_id, &w,
                    &thr, &valid) == 6) {
    const StreamKey key{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)tag};
    std::printf("%08" PRIx32 "\n", noise_word(key, seq_id, w, thr, (uint32_t)valid));
    ++lines;
  }
  return lines > 0 && std::feof(stdin) ? 0 : 1;
}
