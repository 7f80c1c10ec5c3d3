// tip_view.hpp -- where a kernel reads the characters of the tips from (kernels_msa_stats.hpp, kernels_distance.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace pllhip {

// a table of per-tip pointers (a partition) or rows at a fixed stride (an alignment); codes, else vectors in the API
// layout or the 32-site blocked layout (brows != 0)
struct TipView
{
  const uint8_t * const * code_rows;
  const uint8_t * code_base;
  unsigned long long code_stride;
  const double * const * clv_rows;
  unsigned R, Sp, brows;
};

// entry k of rate 0 of site n
__device__ inline double tip_clv(const TipView & tp, unsigned t, unsigned long long n, unsigned k)
{
  return tp.brows ? tp.clv_rows[t][(((n >> 5) * tp.R) * tp.brows + k) * 32 + (n & 31)]
                  : tp.clv_rows[t][n * tp.R * tp.Sp + k];
}

} // namespace pllhip
