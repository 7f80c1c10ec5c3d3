// rell_mix.hpp -- the counter-based generator of the resampling and simulation kernels (kernels_rell.hpp,
// kernels_au.hpp, kernels_simulate.hpp): draw number c of a stream is a function of (seed, c) alone, so the draws do
// not depend on the schedule.
#pragma once
#include <hip/hip_runtime.h>

namespace pllhip {

typedef unsigned long long rell_u64;

// SplitMix64 output number c + 1 of the stream `seed`
__host__ __device__ inline rell_u64 rell_mix(rell_u64 seed, rell_u64 c)
{
  rell_u64 z = seed + (c + 1ULL) * 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

} // namespace pllhip
