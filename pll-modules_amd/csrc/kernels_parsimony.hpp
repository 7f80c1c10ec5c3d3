// kernels_parsimony.hpp -- Fitch parsimony on bit-sliced state sets (pll_fastparsimony_*, pllhip_parsimony_tree_score).
//
// Layout: a vector (the state set of one node over all sites) is [state][word] of uint32, word w holding sites
// 32w .. 32w+31, bit i = site 32w+i.  A partition's vectors live side by side, [node][state][nw]; nw is a
// multiple of 64 so that every lane of every wave owns a real word (padding words are empty sets of weight 0).
// Pattern weights are bit planes: planes[b][w] holds, per site of word w, bit b of its weight, so that the
// weight of the sites in a 32-bit mask m is sum_b popcount(m & planes[b][w]) << b (exact integers).
//
// Every lane owns one word and walks the whole schedule on its own: Fitch never mixes sites, so no lane waits for
// another, and a launch has no inter-workgroup dependency.  A workgroup is one wave; it reduces its per-edge counts
// across the wave and adds them with one integer atomic per edge (order-independent, so bit-reproducible).
// Every loop over states is a streaming loop over memory: no per-lane arrays, nothing that can spill at 64 states.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace pllhip {

constexpr unsigned PARS_WG = 64;        // one wave per workgroup, one word per lane

// schedule of one k_pars_walk launch, int32 in device memory:
//   ndown down ops {parent, child1, child2}: D[parent] = F(D[child1], D[child2]) (parent < 0: the two sets are only
//     joined, for the count); with a score target, each op adds weight x [empty intersection] to it
//   npre preorder ops {v, a, flags, b}: the set above v is U = F(X[a], D[b]) (b < 0: U = X[a]), X = U if flags bit 0
//     else D; flags bit 1: store U as U[v] for v's children.  Edge (v, above v) costs
//     weight x [F(D[v], U) & cand = empty], added to edge_out[op index].
constexpr unsigned PARS_PRE_UP = 1u, PARS_PRE_STORE = 2u;

__device__ inline uint32_t pars_fitch(uint32_t a, uint32_t b, uint32_t nonempty)
{
  return (a & b) | ((a | b) & ~nonempty);
}

__device__ inline unsigned long long pars_weight(uint32_t m, const uint32_t * planes, unsigned nplanes, unsigned nw,
                                                 unsigned w)
{
  unsigned long long c = 0;
  if (m)
    for (unsigned b = 0; b < nplanes; ++b) c += (unsigned long long)__popc(m & planes[(size_t)b * nw + w]) << b;
  return c;
}

__device__ inline unsigned long long pars_wave_sum(unsigned long long c)
{
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  return c;
}

// tip data of the engine -> packed state set of one tip.  One thread per site, one ballot per state: lanes 0 and
// 32 store the two words of the wave.  Sources: coded tips (codes + code -> mask table) or the tip's vector in the
// family's layout (entries > 0: blocked = [block][rate][rows][32], else [site][rate][Sp]); rate 0 only.
// Sites from nreal on (ascertainment-bias columns, padding) are empty.
__global__ __launch_bounds__(PARS_WG) void k_pars_pack(const double * clv, const uint8_t * codes,
                                                        const unsigned long long * tipmap, unsigned blocked,
                                                        unsigned R, unsigned Sp, unsigned rows, unsigned S,
                                                        unsigned nreal, unsigned nw, uint32_t * out)
{
  const unsigned lane = threadIdx.x;
  const unsigned n = blockIdx.x * PARS_WG + lane;
  const bool in = n < nreal;
  const unsigned long long cm = (codes && in) ? tipmap[codes[n]] : 0ULL;
  const size_t base = !in ? 0 : blocked ? ((size_t)(n / 32u) * R * rows) * 32u + (n % 32u) : (size_t)n * R * Sp;
  const size_t step = blocked ? 32u : 1u;
  for (unsigned s = 0; s < S; ++s)
  {
    bool bit = false;
    if (in) bit = codes ? ((cm >> s) & 1ULL) != 0 : clv[base + s * step] > 0.0;
    const unsigned long long m = __ballot(bit);
    if (lane == 0) out[(size_t)s * nw + 2u * blockIdx.x] = (uint32_t)m;
    if (lane == 32) out[(size_t)s * nw + 2u * blockIdx.x + 1u] = (uint32_t)(m >> 32);
  }
}

// One walk over a schedule (see above).  Stepwise addition: the down ops are the path whose sets the last
// insertion changed, the preorder ops every edge of the tree, cand the packed set of the taxon to place.
// Scoring: the down ops of a whole tree plus the final join, no preorder ops.
__global__ __launch_bounds__(PARS_WG) void k_pars_walk(uint32_t * D, uint32_t * U, size_t vec, unsigned S, unsigned nw,
                                                        const uint32_t * planes, unsigned nplanes, const int * ops,
                                                        unsigned ndown, unsigned npre, const uint32_t * cand,
                                                        unsigned long long * edge_out, unsigned long long * score_out)
{
  const unsigned w = blockIdx.x * PARS_WG + threadIdx.x;    // < nw: nw is a multiple of PARS_WG
  unsigned long long score = 0;
  for (unsigned k = 0; k < ndown; ++k)
  {
    const int p = ops[3 * k], c1 = ops[3 * k + 1], c2 = ops[3 * k + 2];
    const uint32_t * x = D + (size_t)c1 * vec + w;
    const uint32_t * y = D + (size_t)c2 * vec + w;
    uint32_t ne = 0;
    for (unsigned s = 0; s < S; ++s) ne |= x[(size_t)s * nw] & y[(size_t)s * nw];
    if (score_out) score += pars_weight(~ne, planes, nplanes, nw, w);
    if (p >= 0)
    {
      uint32_t * o = D + (size_t)p * vec + w;
      for (unsigned s = 0; s < S; ++s) o[(size_t)s * nw] = pars_fitch(x[(size_t)s * nw], y[(size_t)s * nw], ne);
    }
  }
  if (score_out)
  {
    score = pars_wave_sum(score);
    if (threadIdx.x == 0 && score) atomicAdd(score_out, score);
  }
  const int * pre = ops + 3 * ndown;
  for (unsigned e = 0; e < npre; ++e)
  {
    const int v = pre[4 * e], a = pre[4 * e + 1], b = pre[4 * e + 3];
    const unsigned flags = (unsigned)pre[4 * e + 2];
    const uint32_t * xa = ((flags & PARS_PRE_UP) ? U : D) + (size_t)a * vec + w;
    const uint32_t * db = D + (size_t)(b >= 0 ? b : 0) * vec + w;
    const uint32_t * dv = D + (size_t)v * vec + w;
    const uint32_t * ct = cand + w;
    uint32_t * uo = (flags & PARS_PRE_STORE) ? U + (size_t)v * vec + w : nullptr;
    uint32_t ne_up = 0;
    if (b >= 0)
      for (unsigned s = 0; s < S; ++s) ne_up |= xa[(size_t)s * nw] & db[(size_t)s * nw];
    // the set above v, and whether it meets D[v]
    uint32_t ne_edge = 0;
    for (unsigned s = 0; s < S; ++s)
    {
      const uint32_t u = b >= 0 ? pars_fitch(xa[(size_t)s * nw], db[(size_t)s * nw], ne_up) : xa[(size_t)s * nw];
      if (uo) uo[(size_t)s * nw] = u;
      ne_edge |= u & dv[(size_t)s * nw];
    }
    // the edge's set against the candidate
    uint32_t hit = 0;
    for (unsigned s = 0; s < S; ++s)
    {
      const uint32_t u = b >= 0 ? pars_fitch(xa[(size_t)s * nw], db[(size_t)s * nw], ne_up) : xa[(size_t)s * nw];
      hit |= pars_fitch(u, dv[(size_t)s * nw], ne_edge) & ct[(size_t)s * nw];
    }
    const unsigned long long c = pars_wave_sum(pars_weight(~hit, planes, nplanes, nw, w));
    if (threadIdx.x == 0 && c) atomicAdd(edge_out + e, c);
  }
}

// SPR scoring of pruned subtrees (pll_fastparsimony_stepwise_spr_round).  One launch scores B pruned subtrees,
// member m = blockIdx.y; D and U (the current tree's down and up sets) are read-only, every member writes only its
// own scratch, scr + m * scr_stride: the new down sets of the path above the prune point, then the up sets U' of the
// pruned tree T'.  members[m] = {first op, ndown, npre, candidate node, first output}.  An operand is
// (index << 2) | source with source PARS_SRC_D (D[node]), PARS_SRC_U (U[node]) or PARS_SRC_X (scratch slot).
//   ndown down ops {slot, a, b}: X[slot] = F(a, b)
//   npre edge ops {xd, a, b, store, count}: the set above the edge's lower node is u = F(a, b) (b < 0: u = a); with
//     store >= 0 it is kept as X[store]; with count != 0 the edge costs weight x [F(xd, u) & cand = empty], added to
//     out[first output + number of counted ops before it].
constexpr unsigned PARS_SRC_D = 0u, PARS_SRC_U = 1u, PARS_SRC_X = 2u;
constexpr unsigned PARS_SPR_MAX_BATCH = 64u;
constexpr unsigned PARS_MEMBER_INTS = 5u, PARS_SPR_DOWN_INTS = 3u, PARS_SPR_PRE_INTS = 5u;

__device__ inline const uint32_t * pars_src(int o, const uint32_t * D, const uint32_t * U, const uint32_t * X,
                                            size_t vec)
{
  const unsigned src = (unsigned)o & 3u;
  const uint32_t * base = src == PARS_SRC_D ? D : src == PARS_SRC_U ? U : X;
  return base + (size_t)((unsigned)o >> 2) * vec;
}

__global__ __launch_bounds__(PARS_WG) void k_pars_spr(const uint32_t * D, const uint32_t * U, uint32_t * scr,
                                                       size_t scr_stride, size_t vec, unsigned S, unsigned nw,
                                                       const uint32_t * planes, unsigned nplanes, const int * ops,
                                                       const int * members, unsigned long long * out)
{
  const unsigned w = blockIdx.x * PARS_WG + threadIdx.x;    // < nw: nw is a multiple of PARS_WG
  const int * mem = members + PARS_MEMBER_INTS * blockIdx.y;
  const int * op = ops + mem[0];
  const unsigned ndown = (unsigned)mem[1], npre = (unsigned)mem[2];
  uint32_t * X = scr + (size_t)blockIdx.y * scr_stride;
  const uint32_t * ct = D + (size_t)mem[3] * vec + w;
  unsigned long long * o = out + mem[4];
  for (unsigned k = 0; k < ndown; ++k, op += PARS_SPR_DOWN_INTS)
  {
    const uint32_t * x = pars_src(op[1], D, U, X, vec) + w;
    const uint32_t * y = pars_src(op[2], D, U, X, vec) + w;
    uint32_t * r = X + (size_t)op[0] * vec + w;
    uint32_t ne = 0;
    for (unsigned s = 0; s < S; ++s) ne |= x[(size_t)s * nw] & y[(size_t)s * nw];
    for (unsigned s = 0; s < S; ++s) r[(size_t)s * nw] = pars_fitch(x[(size_t)s * nw], y[(size_t)s * nw], ne);
  }
  for (unsigned e = 0; e < npre; ++e, op += PARS_SPR_PRE_INTS)
  {
    const int b = op[2], st = op[3];
    const uint32_t * xd = pars_src(op[0], D, U, X, vec) + w;
    const uint32_t * xa = pars_src(op[1], D, U, X, vec) + w;
    const uint32_t * xb = pars_src(b >= 0 ? b : op[1], D, U, X, vec) + w;
    uint32_t * uo = st >= 0 ? X + (size_t)st * vec + w : nullptr;
    uint32_t ne_up = 0;
    if (b >= 0)
      for (unsigned s = 0; s < S; ++s) ne_up |= xa[(size_t)s * nw] & xb[(size_t)s * nw];
    uint32_t ne_edge = 0;
    for (unsigned s = 0; s < S; ++s)
    {
      const uint32_t u = b >= 0 ? pars_fitch(xa[(size_t)s * nw], xb[(size_t)s * nw], ne_up) : xa[(size_t)s * nw];
      if (uo) uo[(size_t)s * nw] = u;
      ne_edge |= u & xd[(size_t)s * nw];
    }
    if (!op[4]) continue;
    uint32_t hit = 0;
    for (unsigned s = 0; s < S; ++s)
    {
      const uint32_t u = b >= 0 ? pars_fitch(xa[(size_t)s * nw], xb[(size_t)s * nw], ne_up) : xa[(size_t)s * nw];
      hit |= pars_fitch(u, xd[(size_t)s * nw], ne_edge) & ct[(size_t)s * nw];
    }
    const unsigned long long c = pars_wave_sum(pars_weight(~hit, planes, nplanes, nw, w));
    if (threadIdx.x == 0 && c) atomicAdd(o, c);
    ++o;
  }
}

} // namespace pllhip
