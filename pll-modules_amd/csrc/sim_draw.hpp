// sim_draw.hpp -- the draws of the simulation contract ("Simulated alignments"), shared by the kernels
// that follow it (kernels_simulate.hpp, kernels_ancsample.hpp): the key of (seed, replicate, stream), the uniform number
// of a site under a key, and the pick from a cumulated table.
#pragma once
#include <hip/hip_runtime.h>

#include "rell_mix.hpp"

namespace pllhip {

__host__ __device__ inline rell_u64 sim_key(rell_u64 seed, rell_u64 b, unsigned k) { return rell_mix(seed, (b << 32) | k); }
__host__ __device__ inline double sim_u(rell_u64 key, rell_u64 j) { return (double)(rell_mix(key, j) >> 11) * 0x1.0p-53; }

// the number of s in 0 .. n - 2 with cum[s] <= u, by bisection (cum is monotone: its entries were clamped at 0)
template <typename P> __device__ inline unsigned sim_pick(P cum, unsigned n, double u)
{
  unsigned lo = 0, hi = n - 1;
  while (lo < hi)
  {
    const unsigned mid = (lo + hi) >> 1;
    if (cum[mid] > u) hi = mid; else lo = mid + 1;
  }
  return lo;
}

} // namespace pllhip
