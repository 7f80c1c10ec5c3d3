// kernels_simulate.hpp -- alignments drawn from the model along a tree (contract: INTEGRATION.md, "Simulated
// alignments"; design: DESIGN.md section 28; host side: pll_simulate_dev.hip, sim_plan.hpp).
//
// k_sim_cumulate turns the transition matrices the edge program uses, the category weights and the frequencies into
// running sums (left to right, entries below 0 as 0).  k_sim_evolve gives a workgroup a tile of SIM_TILE sites of one
// replicate -- four neighbouring sites per lane, one byte each in a 32-bit word -- and walks the whole edge program
// with it: the states of the inner nodes stay in LDS slots the plan assigned, a word per lane and slot (lane l reads
// and writes word l of a slot: no two lanes of a wave share a bank), and only the requested rows are stored, one
// 32-bit store per lane and row.  Every draw is a counter-based number of (seed, replicate, stream, absolute site),
// so tiles, grids and chunks do not show in the bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"
#include "sim_draw.hpp"

namespace pllhip {

constexpr unsigned SIM_WG = 256;
constexpr unsigned SIM_LANE_SITES = 4;                    // sites per lane: the bytes of one 32-bit word
constexpr unsigned SIM_TILE = SIM_WG * SIM_LANE_SITES;    // sites per workgroup and pass
constexpr unsigned SIM_NO = ~0u;
constexpr unsigned SIM_LDS_BUDGET = 40u << 10;            // per workgroup: four workgroups per CU keep their 160 KiB
constexpr unsigned SIM_MAX_STATES = 256;                  // a state is a byte

// one draw of the edge program (sim_plan.hpp, Step) as the kernel reads it
struct SimStep
{
  unsigned src, dst;        // slots (dst SIM_NO: the child keeps no slot)
  unsigned table;           // position of the edge's matrix among the cumulated ones
  unsigned stream;          // 3 + matrix index
  unsigned row;             // output row of the child (SIM_NO: not asked for)
};

struct SimTables
{
  const double * cum;       // [table][R][S][S]
  const double * cumw;      // [R]
  const double * cumf;      // [R][S]   frequencies of params_indices[c]
  const double * pinv;      // [R]      prop_invar of params_indices[c]
  const uint8_t * alphabet; // [256]    state -> output byte
};

struct SimLaunch
{
  const SimStep * steps;
  unsigned nsteps, slots, root_row;
  unsigned R, S;
  rell_u64 seed, first_site;      // absolute site of column 0
  unsigned first_replicate;       // absolute number of replicate 0
  unsigned replicates, sites, tiles, rows;
  size_t pitch;                   // bytes between rows (a multiple of 4)
  uint8_t * out;                  // [replicate][row][pitch]
};

__device__ inline double sim_clamp(double x) { return x > 0.0 ? x : 0.0; }

// rows [0, nt R S) : row (t, c, s) of cum = running sums of row s of matrix tables[t], category c;
// then R rows of frequencies; then the weights.  One thread per row; plain adds in index order.
__global__ __launch_bounds__(SIM_WG) void k_sim_cumulate(const double * __restrict__ pmat, const double * __restrict__ model,
                                                         unsigned off_weights, unsigned off_pinv, unsigned off_freqs,
                                                         const unsigned * __restrict__ tables, unsigned nt,
                                                         ParamIdxHost params, unsigned R, unsigned S, unsigned Sp,
                                                         double * __restrict__ cum, double * __restrict__ cumw,
                                                         double * __restrict__ cumf, double * __restrict__ pinv)
{
  const unsigned nrows = nt * R * S;
  for (unsigned i = blockIdx.x * SIM_WG + threadIdx.x; i < nrows + R + 1; i += gridDim.x * SIM_WG)
  {
    if (i < nrows)
    {
      const unsigned s = i % S, c = (i / S) % R, t = i / (S * R);
      const double * src = pmat + (((size_t)tables[t] * R + c) * S + s) * Sp;
      double * dst = cum + (size_t)i * S;
      double acc = 0.0;
      for (unsigned k = 0; k < S; ++k) { acc = acc + sim_clamp(src[k]); dst[k] = acc; }
    }
    else if (i < nrows + R)
    {
      const unsigned c = i - nrows;
      const double * src = model + off_freqs + (size_t)params.v[c] * Sp;
      double acc = 0.0;
      for (unsigned k = 0; k < S; ++k) { acc = acc + sim_clamp(src[k]); cumf[(size_t)c * S + k] = acc; }
      pinv[c] = model[off_pinv + params.v[c]];
    }
    else
    {
      double acc = 0.0;
      for (unsigned c = 0; c < R; ++c) { acc = acc + sim_clamp(model[off_weights + c]); cumw[c] = acc; }
    }
  }
}

// grid: x over (tile, replicate) pairs, any size.  Dynamic LDS: [STAGED ? R S S : 0 doubles][slots][SIM_WG words]
// [256 bytes of alphabet].  STAGED: the R x S cumulated rows of the step's matrix are copied into LDS and searched
// there; otherwise they are searched where they lie (tables beyond the budget: they stay L2-resident).
template <bool STAGED>
__global__ __launch_bounds__(SIM_WG) void k_sim_evolve(SimTables T, SimLaunch L)
{
  extern __shared__ __attribute__((aligned(16))) double sim_lds[];
  const unsigned RSS = L.R * L.S * L.S;
  double * lds_tab = sim_lds;
  unsigned * slot = reinterpret_cast<unsigned *>(sim_lds + (STAGED ? RSS : 0u));
  uint8_t * alpha = reinterpret_cast<uint8_t *>(slot + (size_t)L.slots * SIM_WG);
  const unsigned tid = threadIdx.x;
  alpha[tid] = T.alphabet[tid];                   // (SIM_WG == 256 entries)
  __syncthreads();

  const unsigned items = L.tiles * L.replicates;
  for (unsigned item = blockIdx.x; item < items; item += gridDim.x)
  {
    const unsigned tile = item % L.tiles, rep = item / L.tiles;
    const rell_u64 b = (rell_u64)L.first_replicate + rep;
    const unsigned col = tile * SIM_TILE + tid * SIM_LANE_SITES;
    const bool active = col < L.sites;            // (pitch covers the lane's four bytes whenever its first is a site)
    const rell_u64 j0 = L.first_site + col;
    uint8_t * out = L.out + (size_t)rep * L.rows * L.pitch + col;

    // category, invariance and root state of the lane's sites
    const rell_u64 key_c = sim_key(L.seed, b, 0), key_i = sim_key(L.seed, b, 1), key_r = sim_key(L.seed, b, 2);
    unsigned cats = 0, inv = 0, cur = 0;
#pragma unroll
    for (unsigned i = 0; i < SIM_LANE_SITES; ++i)
    {
      const unsigned c = sim_pick(T.cumw, L.R, sim_u(key_c, j0 + i));
      cats |= c << (8 * i);
      if (sim_u(key_i, j0 + i) < T.pinv[c]) inv |= 1u << i;
      cur |= sim_pick(T.cumf + (size_t)c * L.S, L.S, sim_u(key_r, j0 + i)) << (8 * i);
    }
    slot[tid] = cur;                              // the root lives in slot 0
    if (L.root_row != SIM_NO && active)
      *reinterpret_cast<unsigned *>(out + (size_t)L.root_row * L.pitch) =
          alpha[cur & 255u] | (alpha[(cur >> 8) & 255u] << 8) | (alpha[(cur >> 16) & 255u] << 16) | ((unsigned)alpha[cur >> 24] << 24);

    for (unsigned k = 0; k < L.nsteps; ++k)
    {
      const SimStep st = L.steps[k];
      const rell_u64 key = sim_key(L.seed, b, st.stream);
      const double * tab = T.cum + (size_t)st.table * RSS;
      if (STAGED)
      {
        __syncthreads();                          // the last step's searches are over
        for (unsigned i = tid; i < RSS; i += SIM_WG) lds_tab[i] = tab[i];
        __syncthreads();
      }
      const unsigned from = slot[st.src * SIM_WG + tid];
      unsigned to = 0;
#pragma unroll
      for (unsigned i = 0; i < SIM_LANE_SITES; ++i)
      {
        const unsigned ps = (from >> (8 * i)) & 255u, c = (cats >> (8 * i)) & 255u;
        const unsigned row = (c * L.S + ps) * L.S;
        unsigned s = ps;
        if (!((inv >> i) & 1u))
          s = STAGED ? sim_pick(lds_tab + row, L.S, sim_u(key, j0 + i)) : sim_pick(tab + row, L.S, sim_u(key, j0 + i));
        to |= s << (8 * i);
      }
      if (st.dst != SIM_NO) slot[st.dst * SIM_WG + tid] = to;
      if (st.row != SIM_NO && active)
        *reinterpret_cast<unsigned *>(out + (size_t)st.row * L.pitch) =
            alpha[to & 255u] | (alpha[(to >> 8) & 255u] << 8) | (alpha[(to >> 16) & 255u] << 16) | ((unsigned)alpha[to >> 24] << 24);
    }
  }
}

} // namespace pllhip
