// kernels_ancsample.hpp -- one coherent draw of all ancestors from their joint posterior (contract: INTEGRATION.md,
// "Sampled ancestral states"; design: DESIGN.md section 32; host side: pll_ancsample_dev.hip, launch: pll_core.hip).
//
// k_ancsample_walk gives a workgroup a tile of ANCS_WG neighbouring sites and a group of up to ANCS_RC replicates and
// runs the whole program with it: the component (category, invariant or not) from the site-category table of the root
// edge, the root state, then every edge of the plan from the parent's state and the child's conditional vector.  A
// lane keeps its site and loops over the replicates of the group inside every edge, so the rows of a child's unit are
// asked for by one lane again and again while they are hot; the states of the inner nodes stay in LDS slots the plan
// assigned, one byte per replicate in a 64-bit word per lane and slot (lane l reads and writes word l only: no
// barrier after the alphabet is staged).  Every draw is a counter-based number of (seed, replicate, stream, pattern),
// so tiles, groups, grids and chunks do not show in the bytes.
//
// Arithmetic: every product and sum is a single fp64 operation in the order of the contract; the translation unit is
// built without contraction, and the pragma below says so again for this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_job.hpp"
#include "kernels_generic.hpp"
#include "sim_draw.hpp"

#pragma clang fp contract(off)

namespace pllhip {

constexpr unsigned ANCS_WG = 256;
constexpr unsigned ANCS_RC = 8;                 // replicates of a group: their bytes fill a 64-bit word
constexpr unsigned ANCS_NO = ~0u;

// grid: x over (tile, group) pairs, any size.  Dynamic LDS: [slots][ANCS_WG] 64-bit words, 256 bytes of alphabet.
__global__ __launch_bounds__(ANCS_WG) void k_ancsample_walk(AncsOperands O, AncsLaunch L)
{
  extern __shared__ __attribute__((aligned(16))) unsigned long long ancs_lds[];
  unsigned long long * slot = ancs_lds;
  uint8_t * alpha = reinterpret_cast<uint8_t *>(slot + (size_t)L.slots * ANCS_WG);
  const unsigned tid = threadIdx.x;
  alpha[tid] = L.alphabet[tid];                 // (ANCS_WG == 256 entries)
  __syncthreads();

  const unsigned R = O.R, S = O.S, Sp = O.Sp, brows = O.brows;
  const unsigned long long * tipmap = O.tipmap;
  const unsigned groups = (L.replicates + L.per_pass - 1) / L.per_pass;
  const unsigned items = L.tiles * groups;
  const NodeRef root = {L.root.clv, L.root.codes}, other = {L.other.clv, L.other.codes};
  for (unsigned item = blockIdx.x; item < items; item += gridDim.x)
  {
    const unsigned tile = item % L.tiles, grp = item / L.tiles;
    const unsigned col = tile * ANCS_WG + tid;
    if (col >= L.sites) continue;
    const unsigned long long n = (unsigned long long)L.site0 + col;
    const unsigned rep0 = grp * L.per_pass, nrep = min(L.per_pass, L.replicates - rep0);

    // the masses of the 2 R components: w_r A[n][r], w_r B[n][r]
    auto mass = [&](unsigned s) -> double {
      const unsigned r = s >> 1;
      if (s & 1u) return L.B ? O.weights[r] * L.B[(size_t)r * L.plane + n] : 0.0;
      return O.weights[r] * L.A[(size_t)r * L.plane + n];
    };
    double total = 0.0;
    for (unsigned s = 0; s < 2 * R; ++s) total = total + mass(s);
    if (!(total > 0.0) || !isfinite(total))
    {
      // dropped: its bytes stay 0xFF in every replicate
      if (L.dropped && grp == 0 && L.m[n] > 0) atomicAdd(L.dropped, 1ULL);
      continue;
    }
    const int inv_state = O.invariant ? O.invariant[n] : -1;
    uint8_t * out = L.out + col;
    auto put = [&](unsigned rep, unsigned row, unsigned state) {
      out[((size_t)rep * L.rows + row) * L.pitch] = state == 255u ? (uint8_t)255 : alpha[state];
    };

    // component and root state of every replicate of the group
    unsigned long long comps = 0, cur = 0;
    for (unsigned b = 0; b < nrep; ++b)
    {
      const rell_u64 rep = (rell_u64)L.first_replicate + rep0 + b;
      const unsigned k = ancs_pick(2 * R, sim_u(sim_key(L.seed, rep, 0), n), mass);
      const unsigned r = k >> 1, comp = r | ((k & 1u) << 7);
      unsigned state;
      if (k & 1u) state = (unsigned)inv_state & 255u;
      else
      {
        const double * P0 = O.pmat + L.pm0 + (size_t)r * S * Sp;
        const double * pi = O.freqs + (size_t)O.fidx.v[r] * Sp;
        state = ancs_pick(S, sim_u(sim_key(L.seed, rep, 2), n), [&](unsigned i) -> double {
          double t = 0.0;
          for (unsigned j = 0; j < S; ++j) t = t + P0[(size_t)i * Sp + j] * clv_elem(other, tipmap, brows, n, r, j, R, Sp);
          return (pi[i] * clv_elem(root, tipmap, brows, n, r, i, R, Sp)) * t;
        });
      }
      comps |= (unsigned long long)comp << (8 * b);
      cur |= (unsigned long long)state << (8 * b);
      if (L.comp_row != ANCS_NO) out[((size_t)(rep0 + b) * L.rows + L.comp_row) * L.pitch] = (uint8_t)comp;
      if (L.root_row != ANCS_NO) put(rep0 + b, L.root_row, state);
    }
    slot[tid] = cur;                            // the root lives in slot 0

    for (unsigned k = 0; k < L.nsteps; ++k)
    {
      const AncsStep st = L.steps[k];
      const NodeRef child = {st.child.clv, st.child.codes};
      const unsigned long long from = slot[(size_t)st.src * ANCS_WG + tid];
      unsigned long long to = 0;
      for (unsigned b = 0; b < nrep; ++b)
      {
        const unsigned comp = (unsigned)(comps >> (8 * b)) & 255u, a = (unsigned)(from >> (8 * b)) & 255u;
        unsigned state = a;                     // an invariant draw: the same state everywhere
        if (!(comp & 128u))
        {
          const rell_u64 rep = (rell_u64)L.first_replicate + rep0 + b;
          const double * row = O.pmat + st.pm + ((size_t)comp * S + a) * Sp;
          state = ancs_pick(S, sim_u(sim_key(L.seed, rep, st.stream), n), [&](unsigned j) -> double {
            return row[j] * clv_elem(child, tipmap, brows, n, comp, j, R, Sp);
          });
        }
        to |= (unsigned long long)state << (8 * b);
        if (st.row != ANCS_NO) put(rep0 + b, st.row, state);
      }
      if (st.dst != ANCS_NO) slot[(size_t)st.dst * ANCS_WG + tid] = to;
    }
  }
}

} // namespace pllhip
