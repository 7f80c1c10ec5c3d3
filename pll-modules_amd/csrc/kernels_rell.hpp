// kernels_rell.hpp -- resampling of per-pattern log-likelihoods (RELL): the draws, the counts x likelihoods product on
// v_mfma_f64_16x16x4_f64, and the statistics of the replicates (contract: INTEGRATION.md, "Topology tests and
// bootstrap weights"; design: DESIGN.md section 20).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rell_mix.hpp"

namespace pllhip {

typedef double rell_v4d __attribute__((ext_vector_type(4)));

constexpr unsigned RELL_WG = 256;
constexpr unsigned RELL_TILE = 16;        // replicates and trees per matrix tile; rows of C and L are padded to it
constexpr unsigned RELL_TGROUP = 8;       // tree tiles a wave carries per pass over its counts: 128 trees
constexpr unsigned RELL_CHUNK_MIN = 1024; // patterns per chunk up to 64 chunks ...
constexpr unsigned RELL_CHUNKS_MAX = 64;  // ... longer chunks beyond

// patterns per partial sum: a function of the pattern count alone (never of grid, batch or device), a multiple of 16
__host__ __device__ inline unsigned rell_chunk_len(unsigned S)
{
  const unsigned per = (S + RELL_CHUNKS_MAX - 1) / RELL_CHUNKS_MAX;
  const unsigned len = per > RELL_CHUNK_MIN ? per : RELL_CHUNK_MIN;
  return (len + RELL_TILE - 1) / RELL_TILE * RELL_TILE;
}

// Draw k of replicate first_b + blockIdx.y lands on pattern s, cum[s - 1] <= site < cum[s] (cum == nullptr: unit
// weights, s = site); C[blockIdx.y][s] += 1.  The binary search starts from the bucket of the site: first[j] = the
// pattern of site j << shift, j <= (N - 1) >> shift, and first[((N - 1) >> shift) + 1] = S - 1, so the pattern lies in
// first[j] .. first[j + 1] <= S - 1 (site < N = cum[S - 1]).  Integer atomics only: the counts do not depend on the
// schedule.
__global__ __launch_bounds__(RELL_WG) void k_rell_draw(const rell_u64 * __restrict__ cum,
                                                       const unsigned * __restrict__ first, unsigned shift, size_t Sp,
                                                       rell_u64 N, rell_u64 seed, unsigned first_b,
                                                       unsigned * __restrict__ C)
{
  const rell_u64 b = (rell_u64)first_b + blockIdx.y;
  unsigned * row = C + (size_t)blockIdx.y * Sp;
  const rell_u64 stride = (rell_u64)gridDim.x * RELL_WG;
  for (rell_u64 k = (rell_u64)blockIdx.x * RELL_WG + threadIdx.x; k < N; k += stride)
  {
    const rell_u64 site = __umul64hi(rell_mix(seed, (b << 40) | k), N);
    unsigned s;
    if (!cum) s = (unsigned)site;
    else
    {
      const rell_u64 j = site >> shift;
      unsigned lo = first[j], hi = first[j + 1];
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

// P[chunk][16 bt + i][16 tt + j] = sum over the chunk's patterns of C[16 bt + i][s] L[16 tt + j][s].
// grid: x = chunk, y = four replicate tiles (one per wave), z = RELL_TGROUP tree tiles.  Lane 16 q + n holds
// A[row n][k = q] and B[k = q][column n]; it loads patterns s + 4 q .. s + 4 q + 3 of its row of C (one 16-byte
// load) and of L (32 bytes), and k-step j of a 16-pattern group multiplies patterns s + 4 q + j: a fixed order.
// D: register v of lane 16 q + n = replicate 4 v + q, tree n.  Rows of C beyond the batch, rows of L beyond the trees
// and patterns beyond S are zeros (both operands), so no lane is masked.
__global__ __launch_bounds__(RELL_WG) void k_rell_product(const unsigned * __restrict__ C, const double * __restrict__ L,
                                                          size_t Sp, unsigned chunk, unsigned btiles, unsigned ttiles,
                                                          double * __restrict__ P)
{
  const unsigned lane = threadIdx.x & 63u, q = lane >> 4, n = lane & 15u;
  const unsigned bt = blockIdx.y * 4u + (threadIdx.x >> 6);
  if (bt >= btiles) return;
  const size_t s0 = (size_t)blockIdx.x * chunk, s1 = s0 + chunk < Sp ? s0 + chunk : Sp;
  const unsigned tt0 = blockIdx.z * RELL_TGROUP, nt = ttiles - tt0 < RELL_TGROUP ? ttiles - tt0 : RELL_TGROUP;
  const unsigned * crow = C + (size_t)(bt * RELL_TILE + n) * Sp + 4u * q;
  const double * lrow = L + (size_t)(tt0 * RELL_TILE + n) * Sp + 4u * q;
  rell_v4d acc[RELL_TGROUP];
#pragma unroll
  for (unsigned g = 0; g < RELL_TGROUP; ++g) acc[g] = rell_v4d{0.0, 0.0, 0.0, 0.0};
  for (size_t s = s0; s < s1; s += RELL_TILE)
  {
    const uint4 cv = *reinterpret_cast<const uint4 *>(crow + s);
    const double a0 = (double)cv.x, a1 = (double)cv.y, a2 = (double)cv.z, a3 = (double)cv.w;   // exact
#pragma unroll
    for (unsigned g = 0; g < RELL_TGROUP; ++g)
      if (g < nt)
      {
        const double * lp = lrow + (size_t)g * RELL_TILE * Sp + s;
        const double2 l0 = *reinterpret_cast<const double2 *>(lp), l1 = *reinterpret_cast<const double2 *>(lp + 2);
        acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, l0.x, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, l0.y, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, l1.x, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a3, l1.y, acc[g], 0, 0, 0);
      }
  }
  const size_t Tp = (size_t)ttiles * RELL_TILE, rows = (size_t)btiles * RELL_TILE;
#pragma unroll
  for (unsigned g = 0; g < RELL_TGROUP; ++g)
    if (g < nt)
#pragma unroll
      for (unsigned v = 0; v < 4; ++v)
        P[((size_t)blockIdx.x * rows + bt * RELL_TILE + 4u * v + q) * Tp + (tt0 + g) * RELL_TILE + n] = acc[g][v];
}

// R[b][t] = the chunks' partials added in chunk order; b < nb, t < T
__global__ __launch_bounds__(RELL_WG) void k_rell_reduce(const double * __restrict__ P, unsigned nchunks, size_t rows,
                                                         size_t Tp, unsigned nb, unsigned T, double * __restrict__ R)
{
  const size_t i = (size_t)blockIdx.x * RELL_WG + threadIdx.x;
  if (i >= (size_t)nb * T) return;
  const size_t b = i / T, t = i % T;
  double sum = 0.0;
  for (unsigned c = 0; c < nchunks; ++c) sum += P[((size_t)c * rows + b) * Tp + t];
  R[i] = sum;
}

// the smallest index t * S + s of a non-finite L[t][s], t < T (first_bad starts at ~0)
__global__ __launch_bounds__(RELL_WG) void k_rell_flag(const double * __restrict__ L, unsigned T, unsigned S, size_t Sp,
                                                       rell_u64 * first_bad)
{
  const rell_u64 total = (rell_u64)T * S, stride = (rell_u64)gridDim.x * RELL_WG;
  for (rell_u64 i = (rell_u64)blockIdx.x * RELL_WG + threadIdx.x; i < total; i += stride)
  {
    const double v = L[(size_t)(i / S) * Sp + (size_t)(i % S)];
    if (!(fabs(v) <= 1.7976931348623157e308)) atomicMin(first_bad, i);
  }
}

// out[t] = mean over b of X[b][t] (ref < 0) or of X[b][ref] - X[b][t]; one workgroup per column t = blockIdx.x, thread
// i adds rows i, i + 256, ... in order, the 256 sums meet in a fixed tree
__global__ __launch_bounds__(RELL_WG) void k_rell_colmean(const double * __restrict__ X, unsigned B, unsigned T, int ref,
                                                          double * __restrict__ out)
{
  __shared__ double sh[RELL_WG];
  const unsigned t = blockIdx.x;
  double sum = 0.0;
  for (unsigned b = threadIdx.x; b < B; b += RELL_WG)
  {
    const double * x = X + (size_t)b * T;
    sum += ref < 0 ? x[t] : x[ref] - x[t];
  }
  sh[threadIdx.x] = sum;
  __syncthreads();
  for (unsigned w = RELL_WG / 2; w; w >>= 1)
  {
    if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (!threadIdx.x) out[t] = sh[0] / (double)B;
}

// one thread per replicate: its vote for the best tree, its KH and SH comparisons of every tree, and its likelihood
// weights E[b][t] (the caller averages them with k_rell_colmean)
__global__ __launch_bounds__(RELL_WG) void k_rell_counts(const double * __restrict__ R, unsigned B, unsigned T,
                                                         const double * __restrict__ lnl, unsigned best,
                                                         const double * __restrict__ meanR,
                                                         const double * __restrict__ meanD, unsigned * bp, unsigned * kh,
                                                         unsigned * sh, double * __restrict__ E)
{
  const unsigned stride = gridDim.x * RELL_WG;
  for (unsigned b = blockIdx.x * RELL_WG + threadIdx.x; b < B; b += stride)
  {
    const double * r = R + (size_t)b * T;
    double rmax = r[0], M = r[0] - meanR[0];
    unsigned arg = 0;
    for (unsigned t = 1; t < T; ++t)
    {
      if (r[t] > rmax) { rmax = r[t]; arg = t; }
      const double c = r[t] - meanR[t];
      if (c > M) M = c;
    }
    double esum = 0.0;
    for (unsigned t = 0; t < T; ++t) esum += exp(r[t] - rmax);
    atomicAdd(bp + arg, 1u);
    for (unsigned t = 0; t < T; ++t)
    {
      E[(size_t)b * T + t] = exp(r[t] - rmax) / esum;
      const double delta = lnl[best] - lnl[t];
      if ((r[best] - r[t]) - meanD[t] >= delta) atomicAdd(kh + t, 1u);
      if (M - (r[t] - meanR[t]) >= delta) atomicAdd(sh + t, 1u);
    }
  }
}

} // namespace pllhip
