// Counter-based RNG of the sampling kernel (sampling.hip), once: the 64-bit mix and its mapping to a uniform.
// Plain C++17, no HIP constructs (constexpr functions are callable from device code): the host compiler reads it
// too, so csrc/kernels/tests/rng_hash_dump.cpp prints it for tests/test_sampling_reference_cpu.py.
//
// Contract (tests/sampling_reference.py implements the same from this text):
//   hash64(seed, a, b) = splitmix64's finaliser of  seed ^ a * 0x9E3779B97F4A7C15 ^ b * 0xD1B54A32D192ED03
//                        (all arithmetic mod 2^64; the sampler passes a = generation step, b = token id);
//   hash_uniform       = (h + 0.5) * 2^-23  with  h = hash64 >> 41, the hash's top 23 bits.
// h + 0.5 = (2h + 1) / 2 has at most 24 significant bits, so the fp32 sum and product are exact: the 2^23 values
// are (2h + 1) * 2^-24, from 2^-24 to 1 - 2^-24, never 0 and never 1. (With 24 hash bits, (float)h + 0.5f is a
// tie at h = 2^24 - 1 and rounds to 2^24: u = 1.0f, a Gumbel noise of +inf and a token that wins the draw
// whatever its logit.)
#pragma once

#include <stdint.h>

namespace die {

constexpr uint64_t hash64(uint64_t seed, uint64_t a, uint64_t b) {
  uint64_t z = seed ^ (a * 0x9E3779B97F4A7C15ull) ^ (b * 0xD1B54A32D192ED03ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the top 23 bits of a hash -> uniform strictly inside (0, 1)
constexpr float uniform_from_hash(uint64_t z) { return ((float)(z >> 41) + 0.5f) * 0x1p-23f; }

constexpr float hash_uniform(uint64_t seed, uint64_t a, uint64_t b) { return uniform_from_hash(hash64(seed, a, b)); }

static_assert(uniform_from_hash(0ull) == 0x1p-24f && uniform_from_hash(~0ull) == 1.0f - 0x1p-24f,
              "the uniform stays strictly inside (0, 1)");

}  // namespace die
