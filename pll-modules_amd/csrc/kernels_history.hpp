// kernels_history.hpp -- substitution histories along every edge, between the sampled ends of the ancestral draw
// (contract: INTEGRATION.md, "Sampled substitution histories"; design: DESIGN.md section 33; host side:
// pll_history_dev.hip).
//
// k_history_edges reads a staging half the walk kernel has just filled -- per replicate the state index of every node
// and the component of every pattern -- and gives a workgroup one (replicate, edge, tile of HIST_WG patterns) at a
// time, one pattern per lane.  A lane draws the number of jumps of the uniformized chain from the Poisson table of
// (edge, category) weighted by Rpow[k][a][c], then the chain state by state, and finds the time of the j-th event as
// the j-th smallest of the N stateless 32-bit draws by walking their successors: no list is ever stored.  What a lane
// adds is integers only: pattern weights into counts[a][b], weight times a 32-bit time into units[r][a], so the sums
// do not depend on who adds them when.  Up to 64 states a workgroup keeps both tables of its item in LDS and flushes
// the cells that are not zero with 64-bit integer atomics; beyond that the lanes add to memory themselves.
//
// Arithmetic: every product and sum is a single fp64 operation in the order of the contract; the translation unit is
// built without contraction, and the pragma below says so again for this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sim_draw.hpp"

#pragma clang fp contract(off)

namespace pllhip {

constexpr unsigned HIST_WG = 256;
constexpr unsigned HIST_NO = ~0u;
constexpr unsigned HIST_STREAM = 0x40000000u;   // + (matrix << 11) + i: jump count (0) and steps; + 1024 + i: times
constexpr unsigned HIST_MAX_JUMPS = 1023;       // a Poisson table has 1024 entries at most

struct HistEdge
{
  unsigned parent_row = 0, child_row = 0;       // rows of the staging half
  unsigned matrix = 0;
};

struct HistLaunch
{
  uint8_t * half = nullptr;                     // [replicate][rows][pitch]
  unsigned rows = 0, comp_row = 0;
  unsigned change_row = 0;                      // first of `edges` rows of per-site jump counts (~0u: none)
  size_t pitch = 0;
  unsigned reps = 0;                            // replicates of the chunk
  unsigned rep0 = 0;                            // the chunk's first replicate within the call: the row of the tables
  unsigned first_replicate = 0;                 // ... and its absolute number
  unsigned site0 = 0, sites = 0, tiles = 0;     // patterns site0 .. site0 + sites - 1 are columns 0 .. sites - 1
  unsigned edges = 0;
  const HistEdge * edge = nullptr;
  unsigned S = 0, R = 0, kmax = 0;
  const unsigned * slot = nullptr;              // [R]: the power table of category r
  const double * rpow = nullptr;                // [slot][kmax][S][S]
  const unsigned * len = nullptr;               // [edge][R]: entries of the Poisson table
  const unsigned long long * off = nullptr;     // [edge][R]: its first entry
  const double * pois = nullptr;
  const unsigned * m = nullptr;                 // [patterns] pattern weights
  unsigned long long seed = 0;
  unsigned long long * counts = nullptr;        // [replicate of the call][edge][S][S]
  unsigned long long * units = nullptr;         // [replicate of the call][edge][R][S]
  unsigned long long * dropped_edges = nullptr; // [replicate of the call][edge]
};

// the event time draw i of (replicate, matrix, pattern) with its number in the low bits: distinct, ordered as (T, i)
__device__ inline unsigned long long hist_time_key(unsigned long long seed, unsigned long long rep, unsigned base,
                                                   unsigned i, unsigned long long n)
{
  return ((rell_mix(sim_key(seed, rep, base + 1024u + i), n) >> 32) << 10) | i;
}

// grid: x over (replicate, edge, tile) items, any size.  LDS_TABLES: dynamic LDS of (S S + R S) 64-bit words.
template <bool LDS_TABLES> __global__ __launch_bounds__(HIST_WG) void k_history_edges(HistLaunch L)
{
  extern __shared__ __attribute__((aligned(16))) unsigned long long hist_lds[];
  const unsigned tid = threadIdx.x, S = L.S, R = L.R, SS = S * S, cells = SS + R * S;
  const unsigned long long items = (unsigned long long)L.reps * L.edges * L.tiles;
  for (unsigned long long item = blockIdx.x; item < items; item += gridDim.x)
  {
    const unsigned tile = (unsigned)(item % L.tiles), e = (unsigned)(item / L.tiles % L.edges);
    const unsigned b = (unsigned)(item / L.tiles / L.edges);
    const size_t cell = (size_t)(L.rep0 + b) * L.edges + e;
    unsigned long long * g_counts = L.counts + cell * SS, * g_units = L.units + cell * R * S;
    unsigned long long * counts = LDS_TABLES ? hist_lds : g_counts, * units = LDS_TABLES ? hist_lds + SS : g_units;
    if (LDS_TABLES)
    {
      for (unsigned i = tid; i < cells; i += HIST_WG) hist_lds[i] = 0;
      __syncthreads();
    }
    const unsigned col = tile * HIST_WG + tid;
    const uint8_t * rep_rows = L.half + (size_t)b * L.rows * L.pitch;
    const unsigned comp = col < L.sites ? rep_rows[(size_t)L.comp_row * L.pitch + col] : 255u;
    if (comp != 255u)                           // (a dropped site: nothing, and its byte stays 0xFF)
    {
      const HistEdge E = L.edge[e];
      const unsigned long long n = (unsigned long long)L.site0 + col, rep = (unsigned long long)L.first_replicate + b;
      const unsigned long long w = L.m[n];
      const unsigned a = rep_rows[(size_t)E.parent_row * L.pitch + col], c = rep_rows[(size_t)E.child_row * L.pitch + col];
      int real = 0;
      if (!(comp & 128u))                       // (an invariant draw has rate 0: no events, no time)
      {
        const unsigned r = comp, K = L.len[(size_t)e * R + r], base = HIST_STREAM + (E.matrix << 11);
        const double * pois = L.pois + L.off[(size_t)e * R + r];
        const double * rp = L.rpow + (size_t)L.slot[r] * L.kmax * SS, * R1 = rp + SS;
        double total = 0.0;
        if (a < S && c < S)
          for (unsigned k = 0; k < K; ++k) total = total + pois[k] * rp[(size_t)k * SS + a * S + c];
        if (!(total > 0.0) || !isfinite(total))
        {
          real = -1;                            // a dropped edge
          if (w > 0) atomicAdd(L.dropped_edges + cell, 1ULL);
        }
        else
        {
          const unsigned N = min(HIST_MAX_JUMPS, ancs_pick(K, sim_u(sim_key(L.seed, rep, base), n), [&](unsigned k) -> double {
            return pois[k] * rp[(size_t)k * SS + a * S + c];
          }));
          unsigned x = a;
          unsigned long long at = 0;            // the key of the event before this one
          for (unsigned i = 1; i <= N; ++i)
          {
            const double * to = rp + (size_t)(N - i) * SS;
            const unsigned y = ancs_pick(S, sim_u(sim_key(L.seed, rep, base + i), n), [&](unsigned d) -> double {
              return R1[x * S + d] * to[d * S + c];
            });
            // the i-th smallest key: the least one above the (i - 1)-th
            unsigned long long next = ~0ULL;
            for (unsigned l = 1; l <= N; ++l)
            {
              const unsigned long long key = hist_time_key(L.seed, rep, base, l, n);
              if (key > at && key < next) next = key;
            }
            at = next;
            if (y == x) continue;               // a virtual jump
            ++real;
            if (w > 0)
            {
              const unsigned long long wt = w * (at >> 10);
              atomicAdd(counts + x * S + y, w);
              atomicAdd(units + r * S + x, wt);
              atomicAdd(units + r * S + y, 0ULL - wt);
            }
            x = y;
          }
          if (w > 0) atomicAdd(units + r * S + c, w << 32);
        }
      }
      if (L.change_row != HIST_NO && real >= 0)
        L.half[((size_t)b * L.rows + L.change_row + e) * L.pitch + col] = (uint8_t)min(real, 254);
    }
    if (LDS_TABLES)
    {
      __syncthreads();
      for (unsigned i = tid; i < cells; i += HIST_WG)
      {
        const unsigned long long v = hist_lds[i];
        if (v) atomicAdd(i < SS ? g_counts + i : g_units + (i - SS), v);
      }
      __syncthreads();
    }
  }
}

} // namespace pllhip
