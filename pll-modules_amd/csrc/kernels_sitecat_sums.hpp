// kernels_sitecat_sums.hpp -- what is computed from the resident table of a site-category set (kernels_sitecat.hpp
// fills it from an edge, pllhip_sitecat_from_table from the host): planes A[r][plane], B[r][plane] (or null) and c[N]
// (or null: all 0), with the weights w[R] of the call.  g = A + B, T[n] = sum_r w_r g[n][r] (ascending r).
//
//   k_sitecat_posterior   one thread per site, one pass over the planes: post[n][r] = w_r A / T (kept rate-major, only
//                         when asked for), inv = sum_r w_r B / T, rate = sum_r post rho_r, category = the smallest r
//                         with the largest post and that very double, lnl = log T - c 256 ln 2.  T = 0: all zero,
//                         lnl = -inf.
//   k_sitecat_expect      expected[r] = sum_n m_n w_r g / T for up to SITECAT_RC rates starting at r0, and
//                         sum_n m_n lnl[n] (sites with m_n = 0 add nothing, a site with m_n > 0 and T = 0 makes it
//                         -inf), in ONE launch and in a fixed order: thread-strided sums, wave butterfly, four waves
//                         (the order of block_sum_256, kernels_common.hpp), one total per block and quantity, and the
//                         block that draws the last ticket adds the block totals by block index (the order of
//                         k_final_sum) and writes the results where the host reads them.  Bit-identical from run to run
//                         at a given grid.
// Both walk the sites with a grid stride, so a capped grid changes nothing per site.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace pllhip {

constexpr unsigned SITECAT_RC = 16;                       // rates whose sums one k_sitecat_expect launch keeps in registers
constexpr double SITECAT_LN_SCALE = 177.445678223345993274;   // 256 ln 2 (kernels_common.hpp, LN_SCALE)

struct SiteCatTable
{
  const double * A;
  const double * B;        // or null
  const unsigned * c;      // or null
  size_t plane;
  unsigned N, R;
};

struct SiteCatPost
{
  double * rate;           // [N] or null (a set without rates)
  double * inv;            // [N] or null
  uint8_t * category;      // [N]
  double * category_prob;  // [N]
  double * lnl;            // [N]
  double * post;           // [R][plane] or null
};

__device__ inline double sitecat_g(const SiteCatTable & t, unsigned r, unsigned long long n)
{
  const size_t x = (size_t)r * t.plane + n;
  return t.B ? t.A[x] + t.B[x] : t.A[x];
}

__global__ __launch_bounds__(256) void k_sitecat_posterior(SiteCatTable t, const double * w, const double * rho,
                                                           SiteCatPost out)
{
  for (unsigned long long n = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; n < t.N;
       n += (unsigned long long)gridDim.x * blockDim.x)
  {
    double T = 0.0;
    for (unsigned r = 0; r < t.R; ++r) T += w[r] * sitecat_g(t, r, n);
    double rate = 0.0, inv = 0.0, best = 0.0;
    unsigned idx = 0;
    for (unsigned r = 0; r < t.R; ++r)
    {
      const size_t x = (size_t)r * t.plane + n;
      const double p = (T > 0.0) ? (w[r] * t.A[x]) / T : 0.0;
      if (out.post) out.post[x] = p;
      if (rho) rate += p * rho[r];
      if (t.B) inv += w[r] * t.B[x];
      if (p > best) { best = p; idx = r; }           // (`>`: ties go to the smaller index, an all-zero row to 0)
    }
    out.category[n] = (uint8_t)idx;
    out.category_prob[n] = best;
    if (out.rate) out.rate[n] = rate;
    if (out.inv) out.inv[n] = (T > 0.0) ? inv / T : 0.0;
    out.lnl[n] = log(T) - (double)(t.c ? t.c[n] : 0u) * SITECAT_LN_SCALE;
  }
}

__device__ inline double sitecat_wave_sum(double v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// sum over the 256 threads of a block, valid in thread 0; scratch: 4 doubles of LDS
__device__ inline double sitecat_block_sum(double v, double * scratch)
{
  v = sitecat_wave_sum(v);
  const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) scratch[wv] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) s = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
  __syncthreads();
  return s;
}

// block = 256; block_out [SITECAT_RC + 1][gridDim.x]; ticket: one word, zero between launches; dst [SITECAT_RC + 1]:
// expected[r0 + k] at k, the log-likelihood at SITECAT_RC.  m null: every site weighs 1.
__global__ __launch_bounds__(256) void k_sitecat_expect(SiteCatTable t, const double * w, const unsigned * m,
                                                        unsigned r0, double * block_out, unsigned * ticket,
                                                        double * dst)
{
  constexpr unsigned RC = SITECAT_RC, Q = RC + 1;
  __shared__ double scratch[4];
  __shared__ unsigned s_last;
  const unsigned r1 = (r0 + RC < t.R) ? r0 + RC : t.R;
  double acc[RC], ll = 0.0;
#pragma unroll
  for (unsigned k = 0; k < RC; ++k) acc[k] = 0.0;
  for (unsigned long long n = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; n < t.N;
       n += (unsigned long long)gridDim.x * blockDim.x)
  {
    // T in ascending order of r whatever the chunk: the rates below it, the chunk (kept for the second use), the rest
    double T = 0.0, wg[RC];
    for (unsigned r = 0; r < r0; ++r) T += w[r] * sitecat_g(t, r, n);
#pragma unroll
    for (unsigned k = 0; k < RC; ++k)
    {
      wg[k] = (r0 + k < r1) ? w[r0 + k] * sitecat_g(t, r0 + k, n) : 0.0;
      if (r0 + k < r1) T += wg[k];
    }
    for (unsigned r = r1; r < t.R; ++r) T += w[r] * sitecat_g(t, r, n);
    const unsigned mn = m ? m[n] : 1u;
    if (!mn) continue;
    const double md = (double)mn;
    if (T > 0.0)
    {
#pragma unroll
      for (unsigned k = 0; k < RC; ++k) acc[k] += md * (wg[k] / T);
    }
    ll += md * (log(T) - (double)(t.c ? t.c[n] : 0u) * SITECAT_LN_SCALE);
  }
  const unsigned G = gridDim.x, b = blockIdx.x;
#pragma unroll
  for (unsigned q = 0; q < Q; ++q)
  {
    const double tot = sitecat_block_sum(q < RC ? acc[q < RC ? q : 0] : ll, scratch);
    if (threadIdx.x == 0) block_out[(size_t)q * G + b] = tot;
  }
  if (threadIdx.x == 0)
  {
    __threadfence();                                   // the totals before the ticket
    s_last = (atomicAdd(ticket, 1u) == G - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;                                 // block-uniform
  __threadfence();
  for (unsigned q = 0; q < Q; ++q)
  {
    double a = 0.0;
    for (unsigned bb = threadIdx.x; bb < G; bb += 256)
      a += __hip_atomic_load(block_out + (size_t)q * G + bb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double tot = sitecat_block_sum(a, scratch);
    if (threadIdx.x == 0) dst[q] = tot;
  }
  if (threadIdx.x == 0)
  {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence_system();
  }
}

}   // namespace pllhip
