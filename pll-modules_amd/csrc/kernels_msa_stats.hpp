// kernels_msa_stats.hpp -- alignment statistics and empirical model parameters from device-resident tips
// (pll_msa_stats_dev.hip; contract: INTEGRATION.md, "Empirical parameters and alignment statistics"; design:
// DESIGN.md section 15).
//
// One pass over the tips fills one block of 64-bit integer tables (MST_* offsets below); the host does the few
// divisions.  Integer sums do not depend on the order they are made in, so every result is the same from run to run.
//
//   k_mst_tables<SMAX, VPL, CODED>   a lane owns VPL consecutive sites of a tile of 256 * VPL and walks the tips.  Per
//       site it keeps, in registers, cnt[k] = characters that are no gap and contain state k, the gap count and the
//       AND of the masks.  A character of several states that is no gap is rare: its weight goes into the workgroup's
//       A[k][popcount] table in LDS with integer atomics.  Per tile the counts go to LDS, and lanes that own a pair
//       (i, j) -- or a state k, the "diagonal" -- add cnt_i * cnt_j * w (cnt_k * w) over the tile's sites into
//       registers.  At the end a workgroup adds what is not zero to the global tables, one integer atomic each.
//   k_mst_vecfreq                    tips that are true probability vectors: the one floating-point sum,
//       sum of w * v[k] / sum(v), per lane in site order, per workgroup in a fixed tree, one partial per workgroup.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "tip_view.hpp"

namespace pllhip {

constexpr unsigned MST_WG = 256;
constexpr unsigned MST_MAX_STATES = 64;
// the table block, in 64-bit words
constexpr unsigned MST_BAD = 0;       // min over unmapped characters of tip * sites + site (MST_NO_BAD: none)
constexpr unsigned MST_NONBIN = 1;    // != 0: a tip vector holds an entry that is neither 0 nor 1
constexpr unsigned MST_GAPW = 2;      // sum of w over gap characters
constexpr unsigned MST_WSUM = 3;      // sum of w over sites
constexpr unsigned MST_DIAG = 8;      // [64] sum over sites of w * cnt[k]
constexpr unsigned MST_PAIR = MST_DIAG + MST_MAX_STATES;                               // [i < j], row-major
constexpr unsigned MST_AMBIG = MST_PAIR + MST_MAX_STATES * (MST_MAX_STATES - 1) / 2;   // [k][c]: k * 65 + c
constexpr unsigned MST_WORDS = MST_AMBIG + MST_MAX_STATES * (MST_MAX_STATES + 1);
constexpr unsigned long long MST_NO_BAD = ~0ULL;
// per-site flags
constexpr uint8_t MST_FLAG_GAPCOL = 1;   // every character of the column is a gap
constexpr uint8_t MST_FLAG_ONE = 2;      // the AND of the column's masks has exactly one bit

template <int SMAX> struct MstShape
{
  static constexpr unsigned TASKS = SMAX * (SMAX - 1) / 2 + SMAX;             // pairs, then the diagonal
  static constexpr unsigned PER_LANE = (TASKS + MST_WG - 1) / MST_WG;
  static constexpr unsigned CNT_WORDS = SMAX > 32 ? 4096 : 8192;              // the count tile in LDS
};

__device__ inline unsigned long long mst_wave_sum(unsigned long long v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int SMAX, int VPL, bool CODED>
__global__ __launch_bounds__(MST_WG) void k_mst_tables(TipView tp, const unsigned long long * __restrict__ tipmap,
                                                       const unsigned * __restrict__ weights, unsigned T, unsigned N,
                                                       unsigned S, unsigned long long * __restrict__ out,
                                                       uint8_t * __restrict__ flags,
                                                       unsigned long long * __restrict__ seq_gap)
{
  using Shape = MstShape<SMAX>;
  constexpr unsigned TILE = MST_WG * VPL;
  constexpr unsigned SPR = (Shape::CNT_WORDS / SMAX) < TILE ? (Shape::CNT_WORDS / SMAX) : TILE;   // sites per round
  constexpr unsigned ROUNDS = TILE / SPR;
  __shared__ unsigned sCnt[SMAX * SPR];
  __shared__ unsigned sW[SPR];
  __shared__ unsigned long long sA[SMAX * (SMAX + 1)];
  __shared__ unsigned long long sMap[CODED ? 256 : 1];
  __shared__ unsigned short sTask[Shape::TASKS];

  const unsigned tid = threadIdx.x;
  const unsigned long long full = S < 64 ? ((1ULL << S) - 1ULL) : ~0ULL;
  const unsigned ntasks = S * (S - 1) / 2 + S;
  for (unsigned i = tid; i < SMAX * (SMAX + 1); i += MST_WG) sA[i] = 0;
  if constexpr (CODED) sMap[tid] = tipmap[tid];
  // task p: a pair (i, j), i < j, in row-major order, then the states (i, i)
  for (unsigned p = tid; p < ntasks; p += MST_WG)
  {
    unsigned i = 0, j = 0;
    if (p >= S * (S - 1) / 2) i = j = p - S * (S - 1) / 2;
    else
    {
      unsigned q = p;
      while (q >= S - 1 - i) { q -= S - 1 - i; ++i; }
      j = i + 1 + q;
    }
    sTask[p] = (unsigned short)(i | (j << 8));
  }
  __syncthreads();

  unsigned long long acc[Shape::PER_LANE];
#pragma unroll
  for (unsigned q = 0; q < Shape::PER_LANE; ++q) acc[q] = 0;
  unsigned long long gap_w = 0, w_sum = 0;

  const unsigned ntiles = (N + TILE - 1) / TILE;
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
  {
    const unsigned long long n0 = (unsigned long long)tile * TILE + (unsigned long long)tid * VPL;
    unsigned cnt[VPL][SMAX];
    unsigned gaps[VPL], w[VPL];
    unsigned long long common[VPL];
    bool live[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v)
    {
      live[v] = n0 + v < N;
      w[v] = live[v] ? (weights ? weights[n0 + v] : 1u) : 0u;
      gaps[v] = 0;
      common[v] = ~0ULL;
      w_sum += w[v];
#pragma unroll
      for (int k = 0; k < SMAX; ++k) cnt[v][k] = 0;
    }
    for (unsigned t = 0; t < T; ++t)
    {
      unsigned long long m[VPL];
      bool gap[VPL];
      if (CODED)
      {
        const uint8_t * row = tp.code_rows ? tp.code_rows[t] : tp.code_base + (unsigned long long)t * tp.code_stride;
        unsigned chars = 0;
        if (VPL == 4 && n0 + 4 <= N) chars = *reinterpret_cast<const unsigned *>(row + n0);
        else
        {
#pragma unroll
          for (int v = 0; v < VPL; ++v) if (live[v]) chars |= (unsigned)row[n0 + v] << (8 * v);
        }
#pragma unroll
        for (int v = 0; v < VPL; ++v)
        {
          const unsigned long long raw = sMap[(chars >> (8 * v)) & 255u];
          if (live[v] && !raw) atomicMin(out + MST_BAD, (unsigned long long)t * N + n0 + v);
          m[v] = live[v] ? (raw & full) : 0ULL;
          gap[v] = live[v] && m[v] == full;
        }
      }
      else
      {
#pragma unroll
        for (int v = 0; v < VPL; ++v)
        {
          m[v] = 0;
          bool all_set = live[v], other = false;
          if (live[v])
            for (unsigned k = 0; k < S; ++k)            // (no per-lane array here: the bits go into one register pair)
            {
              const double x = tip_clv(tp, t, n0 + v, k);
              if (x > 0.0) m[v] |= 1ULL << k;
              if (x < 1e-7) all_set = false;
              if (x != 0.0 && x != 1.0) other = true;
            }
          gap[v] = all_set;
          if (other) out[MST_NONBIN] = 1;               // (every writer stores the same value)
        }
      }
      unsigned long long gw = 0;
#pragma unroll
      for (int v = 0; v < VPL; ++v)
      {
        if (live[v]) common[v] &= m[v];
        gaps[v] += gap[v] ? 1u : 0u;
        gw += gap[v] ? w[v] : 0u;
        const unsigned long long me = gap[v] ? 0ULL : m[v];
        const unsigned lo = (unsigned)me, hi = (unsigned)(me >> 32);
#pragma unroll
        for (int k = 0; k < SMAX; ++k) cnt[v][k] += ((k < 32 ? lo : hi) >> (k & 31)) & 1u;
        const unsigned c = (unsigned)__popcll(me);
        if (c >= 2)                                     // rare: an ambiguity code that is no gap
          for (unsigned long long rest = me; rest; rest &= rest - 1)
            atomicAdd(&sA[(unsigned)__builtin_ctzll(rest) * (SMAX + 1) + c], (unsigned long long)w[v]);
      }
      gap_w += gw;
      if (seq_gap && __ballot(gw != 0))
      {
        const unsigned long long tot = mst_wave_sum(gw);
        if ((tid & 63u) == 0) atomicAdd(seq_gap + t, tot);
      }
    }
    if (flags)
    {
#pragma unroll
      for (int v = 0; v < VPL; ++v)
        if (live[v])
          flags[n0 + v] = (uint8_t)((gaps[v] == T ? MST_FLAG_GAPCOL : 0) | (__popcll(common[v]) == 1 ? MST_FLAG_ONE : 0));
    }
    // the counts of the tile to LDS, SPR sites at a time; then every task over those sites
#pragma unroll
    for (unsigned r = 0; r < ROUNDS; ++r)
    {
      __syncthreads();
#pragma unroll
      for (int v = 0; v < VPL; ++v)
      {
        const unsigned slot = tid * VPL + v - r * SPR;      // (wraps below zero for the lanes of later rounds)
        if (slot < SPR)
        {
          sW[slot] = w[v];
#pragma unroll
          for (int k = 0; k < SMAX; ++k) sCnt[k * SPR + slot] = cnt[v][k];
        }
      }
      __syncthreads();
#pragma unroll
      for (unsigned q = 0; q < Shape::PER_LANE; ++q)
      {
        const unsigned p = tid + q * MST_WG;
        if (p < ntasks)
        {
          const unsigned ij = sTask[p], i = ij & 255u, j = ij >> 8;
          unsigned long long sum = 0;
          // lanes start at different sites: the rows of two lanes are a multiple of 32 words apart
          for (unsigned s = 0; s < SPR; ++s)
          {
            const unsigned slot = (s + tid) & (SPR - 1);
            const unsigned long long a = sCnt[i * SPR + slot];
            const unsigned long long b = i == j ? 1ULL : sCnt[j * SPR + slot];
            sum += a * b * sW[slot];
          }
          acc[q] += sum;
        }
      }
    }
  }

  // flush: what is not zero, one integer atomic each
  __syncthreads();
#pragma unroll
  for (unsigned q = 0; q < Shape::PER_LANE; ++q)
  {
    const unsigned p = tid + q * MST_WG;
    if (p < ntasks && acc[q])
    {
      const unsigned npairs = S * (S - 1) / 2;
      atomicAdd(out + (p < npairs ? MST_PAIR + p : MST_DIAG + (p - npairs)), acc[q]);
    }
  }
  for (unsigned i = tid; i < SMAX * (SMAX + 1); i += MST_WG)
    if (sA[i]) atomicAdd(out + MST_AMBIG + (i / (SMAX + 1)) * (MST_MAX_STATES + 1) + i % (SMAX + 1), sA[i]);
  gap_w = mst_wave_sum(gap_w);
  w_sum = mst_wave_sum(w_sum);
  if ((tid & 63u) == 0)
  {
    if (gap_w) atomicAdd(out + MST_GAPW, gap_w);
    if (w_sum) atomicAdd(out + MST_WSUM, w_sum);
  }
}

// partial[block][k] = sum over the block's sites and all tips of w * v[k] / sum(v).  A lane owns one state of one
// site: KP (a power of two >= S, <= 64) neighbouring lanes hold a character, sum(v) is a butterfly over them, a lane
// adds its sites in ascending order (tips inside), and the lanes of a block that own the same state are added in a
// fixed tree.  The same grid gives the same bits.
__global__ __launch_bounds__(MST_WG) void k_mst_vecfreq(TipView tp, const unsigned * __restrict__ weights, unsigned T,
                                                        unsigned N, unsigned S, unsigned KP,
                                                        double * __restrict__ partial)
{
  __shared__ double sRed[MST_WG];
  const unsigned tid = threadIdx.x, k = tid & (KP - 1u), per_block = MST_WG / KP;
  double f = 0.0;
  for (unsigned long long n = (unsigned long long)blockIdx.x * per_block + tid / KP; n < N;
       n += (unsigned long long)gridDim.x * per_block)
  {
    const double w = (double)weights[n];
    for (unsigned t = 0; t < T; ++t)
    {
      const double x = k < S ? tip_clv(tp, t, n, k) : 0.0;
      double sum = x;
      for (unsigned off = KP >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, (int)off, 64);
      f += w * x / sum;
    }
  }
  sRed[tid] = f;
  __syncthreads();
  for (unsigned half = MST_WG / 2; half >= KP; half >>= 1)
  {
    if (tid < half) sRed[tid] += sRed[tid + half];
    __syncthreads();
  }
  if (tid < S) partial[(unsigned long long)blockIdx.x * S + tid] = sRed[tid];
}

} // namespace pllhip
