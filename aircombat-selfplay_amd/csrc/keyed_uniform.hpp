// The library's keyed counter-based generator, compiled for the device and the host: the policies' sampling draws (policy_kernel.hpp,
// ac_policy_draw_host) and the spawn curriculum's entry draws (spawn_bank.hpp, ac_spawn_draw_host) are this one function.
#pragma once

namespace pol {
// a pure function of (seed, counter, row, head), uniform on [0, 1) in steps of 2^-24
__host__ __device__ __forceinline__ unsigned long long policy_mix(unsigned long long z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL; z ^= z >> 27; z *= 0x94D049BB133111EBULL; z ^= z >> 31;
  return z;
}
__host__ __device__ __forceinline__ float policy_uniform(unsigned long long seed, unsigned long long counter, long long row, int head) {
  unsigned long long z = policy_mix(seed * 0x9E3779B97F4A7C15ULL + 0x6A09E667F3BCC909ULL);
  z = policy_mix(z ^ (counter * 0xD1B54A32D192ED03ULL));
  z = policy_mix(z ^ (((unsigned long long)row << 8) | (unsigned long long)(head & 0xff)));
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}
}  // namespace pol
