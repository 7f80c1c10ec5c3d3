// kernels_au.hpp -- the approximately unbiased (AU) test from multiscale bootstrap replicates: draws whose rows carry
// their own stream and length, the per-scale bootstrap proportions, and the weighted least-squares fit of the (d, c)
// curve per tree.  The replicate log-likelihoods come from k_rell_product / k_rell_reduce (kernels_rell.hpp).
// Contract: INTEGRATION.md, "Topology tests and bootstrap weights"; design: DESIGN.md section 25.
#pragma once
#include "kernels_rell.hpp"

namespace pllhip {

// one row of a pass: replicate b of scale k draws n sites from the stream `seed` (= rell_mix(~seed of the call, k))
struct au_row
{
  rell_u64 seed;
  rell_u64 n;
  unsigned b;
  unsigned k;
};

__host__ __device__ inline rell_u64 au_scale_seed(rell_u64 seed, unsigned k) { return rell_mix(~seed, k); }

// k_rell_draw with the row's description read from rows[blockIdx.y]: draw j < n of the row lands on the pattern of
// site mulhi64(mix(seed, (b << 40) | j), N).  N bounds the site, and with it the bucket and the search (site < N =
// cum[S - 1]); n only bounds the loop, so rows of different lengths share a launch and the short ones fall out of the
// grid-stride loop.  Integer atomics only.
__global__ __launch_bounds__(RELL_WG) void k_au_draw(const rell_u64 * __restrict__ cum,
                                                     const unsigned * __restrict__ first, unsigned shift, size_t Sp,
                                                     rell_u64 N, const au_row * __restrict__ rows,
                                                     unsigned * __restrict__ C)
{
  const au_row r = rows[blockIdx.y];
  const rell_u64 high = (rell_u64)r.b << 40;
  unsigned * row = C + (size_t)blockIdx.y * Sp;
  const rell_u64 stride = (rell_u64)gridDim.x * RELL_WG;
  for (rell_u64 j = (rell_u64)blockIdx.x * RELL_WG + threadIdx.x; j < r.n; j += stride)
  {
    const rell_u64 site = __umul64hi(rell_mix(r.seed, high | j), N);
    unsigned s;
    if (!cum) s = (unsigned)site;
    else
    {
      const rell_u64 bucket = site >> shift;
      unsigned lo = first[bucket], hi = first[bucket + 1];
      while (lo < hi)
      {
        const unsigned mid = lo + (hi - lo) / 2;
        if (cum[mid] > site) hi = mid; else lo = mid + 1;
      }
      s = lo;
    }
    atomicAdd(row + s, 1u);
  }
}

// one thread per row of R[nb][T]: the first maximum over the trees votes in bp[k of the row][t]
__global__ __launch_bounds__(RELL_WG) void k_au_counts(const double * __restrict__ R,
                                                       const au_row * __restrict__ rows, unsigned nb, unsigned T,
                                                       unsigned * bp)
{
  const unsigned i = blockIdx.x * RELL_WG + threadIdx.x;
  if (i >= nb) return;
  const double * r = R + (size_t)i * T;
  double rmax = r[0];
  unsigned arg = 0;
  for (unsigned t = 1; t < T; ++t)
    if (r[t] > rmax) { rmax = r[t]; arg = t; }
  atomicAdd(bp + (size_t)rows[i].k * T + arg, 1u);
}

// sqrt 2 erfcinv(2 p), the upper-tail quantile of the normal distribution.  Not inlined: inside k_au_fit's loop over the
// scales the compiler would keep the coefficients of every branch of erfcinv in registers across the loop (255 VGPRs
// and 190 AGPRs by the compiler's resource remarks); with the call the kernel needs 74 VGPRs and still no scratch.
__device__ __noinline__ double au_upper_quantile(double p) { return 1.4142135623730951 * erfcinv(2.0 * p); }

// one thread per tree: z_k ~ d sqrt(rho_k) + c / sqrt(rho_k) by weighted least squares over the usable scales
// (0 < count < B), in scale order; fewer than two usable scales: p_au = bp[kstar][t] / B and zeros.  z_k = -Phi^-1(p_k)
// comes from the smaller tail, sqrt 2 erfcinv(2 min(p, 1 - p)) with the sign of 1/2 - p; its weight is
// B phi(z)^2 / (p (1 - p)).  Pass 0 over the scales accumulates the normal equations, pass 1 the residuals; both go
// through the same loop body, so the thread keeps no array and erfcinv is expanded once.
__global__ __launch_bounds__(RELL_WG) void k_au_fit(const unsigned * __restrict__ bp, const double * __restrict__ rho,
                                                    unsigned K, unsigned T, unsigned B, unsigned kstar,
                                                    double * __restrict__ p_au, double * __restrict__ d_out,
                                                    double * __restrict__ c_out, double * __restrict__ se,
                                                    double * __restrict__ rss, unsigned * __restrict__ used)
{
  const unsigned t = blockIdx.x * RELL_WG + threadIdx.x;
  if (t >= T) return;
  double a11 = 0.0, a12 = 0.0, a22 = 0.0, b1 = 0.0, b2 = 0.0, det = 0.0, d = 0.0, c = 0.0, sum = 0.0;
  unsigned n = 0;
#pragma nounroll
  for (unsigned pass = 0; pass < 2; ++pass)
  {
#pragma nounroll
    for (unsigned k = 0; k < K; ++k)
    {
      const unsigned count = bp[(size_t)k * T + t];
      if (!count || count >= B) continue;
      const bool lower = 2u * count <= B;
      const double p = (double)count / (double)B, q = (double)(B - count) / (double)B;
      const double tail = au_upper_quantile(lower ? p : q), z = lower ? tail : -tail;
      const double phi = exp(-(z * z) / 2.0) / 2.5066282746310002, w = (double)B * (phi * phi) / (p * q);
      const double x1 = sqrt(rho[k]), x2 = 1.0 / x1;
      if (!pass)
      {
        a11 += w * (x1 * x1);
        a12 += w * (x1 * x2);
        a22 += w * (x2 * x2);
        b1 += w * (x1 * z);
        b2 += w * (x2 * z);
        ++n;
      }
      else
      {
        const double e = z - (d * x1 + c * x2);
        sum += w * (e * e);
      }
    }
    if (pass) break;
    used[t] = n;
    if (n < 2)
    {
      p_au[t] = (double)bp[(size_t)kstar * T + t] / (double)B;
      d_out[t] = c_out[t] = se[t] = rss[t] = 0.0;
      return;
    }
    det = a11 * a22 - a12 * a12;
    d = (a22 * b1 - a12 * b2) / det;
    c = (a11 * b2 - a12 * b1) / det;
  }
  const double x = d - c;
  p_au[t] = 1.0 - erfc(-x / 1.4142135623730951) / 2.0;
  d_out[t] = d;
  c_out[t] = c;
  se[t] = exp(-(x * x) / 2.0) / 2.5066282746310002 * sqrt((a11 + a22 + 2.0 * a12) / det);
  rss[t] = sum;
}

} // namespace pllhip
