// sim_draw.hpp -- the draws of the simulation contract ("Simulated alignments"), shared by the kernels
// that follow it (kernels_simulate.hpp, kernels_ancsample.hpp): the key of (seed, replicate, stream), the uniform number
// of a site under a key, and the pick from a cumulated table or from masses that are never stored.
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

// pick(u total, cum) over the n masses term(0) .. term(n - 1), cumulated left to right from 0.0: the bisection of
// sim_pick.  The table is never stored: where no mass is negative the running sums do not fall, and the bisection ends
// at the number of s in 0 .. n - 2 whose sum is not above the draw; otherwise the bisection is walked as it stands,
// every probe cumulated anew (the same additions, hence the same sums).
template <class Term> __device__ inline unsigned ancs_pick(unsigned n, double u, Term term)
{
#pragma clang fp contract(off)
  double total = 0.0;
  bool monotone = true;
  for (unsigned s = 0; s < n; ++s)
  {
    const double m = term(s);
    monotone = monotone && m >= 0.0;
    total = total + m;
  }
  const double x = u * total;
  if (monotone)
  {
    double acc = 0.0;
    unsigned s = 0;
    for (; s + 1 < n; ++s)
    {
      acc = acc + term(s);
      if (acc > x) break;
    }
    return s;
  }
  unsigned lo = 0, hi = n - 1;
  while (lo < hi)
  {
    const unsigned mid = (lo + hi) >> 1;
    double acc = 0.0;
    for (unsigned s = 0; s <= mid; ++s) acc = acc + term(s);
    if (acc > x) hi = mid; else lo = mid + 1;
  }
  return lo;
}

} // namespace pllhip
