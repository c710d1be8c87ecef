// Prints rng_hash.h's hash and uniform for tests/test_sampling_reference_cpu.py. Arguments: any number of
// "seed step token" triples (decimal, unsigned 64-bit); one line per triple: the 64-bit hash in hex, then the bit
// pattern of the fp32 uniform in hex. With "raw" before a value, that value is taken as the hash itself
// (the smallest and largest h).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../rng_hash.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc;) {
    uint64_t z;
    if (std::strcmp(argv[i], "raw") == 0) {
      if (i + 1 >= argc) return 2;
      z = std::strtoull(argv[i + 1], nullptr, 0);
      i += 2;
    } else {
      if (i + 2 >= argc) return 2;
      z = die::hash64(std::strtoull(argv[i], nullptr, 0), std::strtoull(argv[i + 1], nullptr, 0),
                      std::strtoull(argv[i + 2], nullptr, 0));
      i += 3;
    }
    const float u = die::uniform_from_hash(z);
    uint32_t bits;
    std::memcpy(&bits, &u, sizeof bits);
    std::printf("%016" PRIx64 " %08" PRIx32 "\n", z, bits);
  }
  return 0;
}
