// kernels_ancestral.hpp -- marginal ancestral states of a node, batched and device-resident
// (pllhip_node_ancestral_batch; the per-call form pll_compute_node_ancestral keeps k_node_ancestral).
//
// Value per site n and state i, as src/tree/treeinfo.c:1698 defines it:
//     a[i] = sum_r w_r pi_r[i] node[n, r, i] * sum_j P_r[i][j] other[n, r, j],   probs[n][i] = a[i] / sum_i a[i]
// (scaler counts and p-inv ignored; a site whose sum is 0 keeps an all-zero row), plus the summary most callers
// want: states[n] = smallest i with the largest probs[n][i], state_probs[n] = that value -- taken from the very
// doubles `probs` holds, so states == argmax(probs) exactly.
//
//   k_anc_s20 / k_anc_s16   blocked families: a wave owns a 32-site block and walks its rates.  P_r * other on the
//                           matrix cores with the family's addressing: a unit of `other` is the B operand (one
//                           coalesced 1 KiB load per k-step), the D rows come out in the address form of the node's
//                           unit, so the Hadamard product with node[n, r, .] needs no shuffle.  A coded `other` reads
//                           its row of the matrix's tip lookup table instead.  The sum over rates stays in registers;
//                           the per-site sum and the argmax run over the state rows of a lane, then over the four q
//                           lane groups (xor-16 / xor-32 shuffles, ties to the smaller index).  Summaries are stored
//                           by the q = 0 lanes (16 B and 2 B per lane, contiguous over the block); the full table goes
//                           through a wave-private LDS tile (transposed to [site][state]) and leaves as the block's
//                           contiguous 32 S doubles.  Padding sites of the last block are never written.
//                           The 20-state family's fragments and units are those of the general family at five
//                           k-steps (same tail instruction for rows 16 .. 19), so both kernels share one body.
//   k_anc_s4                API layout: one thread per site, the 4 x 4 products in registers, 32-byte row stores.
//   k_anc_generic           every other family (33 .. 64 states, the generic layout): the arithmetic of
//                           k_node_ancestral into the batch's table, then k_anc_summary per site.
#pragma once

#include "kernels_common.hpp"
#include "kernels_generic.hpp"
#include "kernels_s4.hpp"
#include "kernels_s20.hpp"
#include "kernels_s16.hpp"

namespace pllhip {

struct AncOut
{
  uint8_t * states;        // [N]
  double * state_probs;    // [N]
  double * probs;          // [N][S] or null
};

// row stride of the LDS tile of a block: odd, so that the sites of a wave's lanes spread over the banks
__host__ __device__ inline unsigned anc_tile_stride(unsigned S) { return S | 1u; }

// LDS doubles of the blocked kernels: the A fragments of all rates, and one tile per wave for the full table
template <unsigned KS>
__host__ __device__ inline unsigned anc_blocked_lds(unsigned R, unsigned S, bool probs)
{
  return R * s16_fr(KS) + (probs ? 4u * S20_BS * anc_tile_stride(S) : 0u);
}

template <unsigned KS>
__device__ inline void anc_blocked_body(const ModelView & mv, const ParamIdx & fidx, const NodeRef & node,
                                        const NodeRef & other, const double * pmat, const double * lut,
                                        unsigned lut_codes, const unsigned long long * tipmap, unsigned N,
                                        unsigned nblk, unsigned R, const AncOut & out, double * lds)
{
  constexpr unsigned UNIT = 4 * KS * S20_BS;
  const unsigned S = mv.S;
  double * frag = lds;
  if (!other.codes) s16_fill_frags<KS>(frag, pmat, R, S, mv.Sp);
  __syncthreads();

  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned q = lane >> 4, n = lane & 15;
  const unsigned wstride = gridDim.x * 4;
  const unsigned TS = anc_tile_stride(S);
  double * tile = lds + R * s16_fr(KS) + wave * S20_BS * TS;

  for (unsigned blk = blockIdx.x * 4 + wave; blk < nblk; blk += wstride)
  {
    const size_t site0 = (size_t)blk * S20_BS + 2 * n;
    unsigned oce = 0, oco = 0;
    unsigned long long nme = 0, nmo = 0;
    if (other.codes) { oce = other.codes[site0]; oco = other.codes[site0 + 1]; }
    if (node.codes) { nme = tipmap[node.codes[site0]]; nmo = tipmap[node.codes[site0 + 1]]; }
    double2 acc[KS];
#pragma unroll
    for (unsigned v = 0; v < KS; ++v) acc[v] = make_double2(0.0, 0.0);
    for (unsigned r = 0; r < R; ++r)
    {
      const size_t ubase = ((size_t)blk * R + r) * UNIT;
      const double * pi = mv.freqs(fidx.v[r]);
      const double w = mv.weights()[r];
      double2 t[KS], pv[KS];
      if (other.codes) s16_child_tip<KS>(lut + (size_t)r * lut_codes * S, oce, oco, q, S, t);
      else s16_child_inner<KS>(other.clv + ubase, frag + r * s16_fr(KS), lane, t);
      if (node.codes) s16_tip_d<KS>(nme, nmo, q, S, pv);
      else s16_load_d<KS>(node.clv + ubase, lane, pv);
#pragma unroll
      for (unsigned v = 0; v < KS; ++v)
      {
        const unsigned i = 4 * v + q;
        const double f = (i < S) ? w * pi[i] : 0.0;
        acc[v].x += f * pv[v].x * t[v].x;
        acc[v].y += f * pv[v].y * t[v].y;
      }
    }
    // per-site sum: the rows of this lane, then the four q groups (every lane ends with the same total)
    double se = 0.0, so = 0.0;
#pragma unroll
    for (unsigned v = 0; v < KS; ++v)
      if (4 * v + q < S) { se += acc[v].x; so += acc[v].y; }
    se = s20_sum_q(se);
    so = s20_sum_q(so);
    // normalise, argmax over the lane's rows (ascending: `>` keeps the smaller index)
    double be = -1.0, bo = -1.0;
    unsigned ie = 0xffffffffu, io = 0xffffffffu;
#pragma unroll
    for (unsigned v = 0; v < KS; ++v)
    {
      const unsigned i = 4 * v + q;
      if (se > 0.0) acc[v].x /= se;
      if (so > 0.0) acc[v].y /= so;
      if (i < S)
      {
        if (acc[v].x > be) { be = acc[v].x; ie = i; }
        if (acc[v].y > bo) { bo = acc[v].y; io = i; }
      }
    }
#pragma unroll
    for (unsigned m = 16; m <= 32; m <<= 1)
    {
      const double xe = __shfl_xor(be, m, 64), xo = __shfl_xor(bo, m, 64);
      const unsigned je = __shfl_xor(ie, m, 64), jo = __shfl_xor(io, m, 64);
      if (xe > be || (xe == be && je < ie)) { be = xe; ie = je; }
      if (xo > bo || (xo == bo && jo < io)) { bo = xo; io = jo; }
    }
    if (q == 0 && site0 < N)
    {
      if (site0 + 1 < N)
      {
        // (site0 is even and the arrays are 16-byte aligned: one 2-byte and one 16-byte store per lane)
        *reinterpret_cast<unsigned short *>(out.states + site0) = (unsigned short)(ie | (io << 8));
        *reinterpret_cast<double2 *>(out.state_probs + site0) = make_double2(be, bo);
      }
      else
      {
        out.states[site0] = (uint8_t)ie;
        out.state_probs[site0] = be;
      }
    }
    if (out.probs)
    {
      // [state row][site] registers -> [site][state] tile -> the block's contiguous run of the table
#pragma unroll
      for (unsigned v = 0; v < KS; ++v)
      {
        const unsigned i = 4 * v + q;
        if (i < S)
        {
          tile[(2 * n) * TS + i] = acc[v].x;
          tile[(2 * n + 1) * TS + i] = acc[v].y;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const size_t first = (size_t)blk * S20_BS;
      const unsigned live = (unsigned)((N - first < S20_BS) ? N - first : S20_BS);
      double * dst = out.probs + first * S;
      for (unsigned x = lane; x < live * S; x += 64)
      {
        const unsigned s = x / S, i = x - s * S;
        dst[x] = tile[s * TS + i];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// grid = min(ceil(nblk / 4), a few per CU), block = 256; dynamic LDS = anc_blocked_lds<KS>() doubles
__global__ __launch_bounds__(256) void k_anc_s20(ModelView mv, ParamIdx fidx, NodeRef node, NodeRef other,
                                                 const double * pmat, const double * lut, unsigned lut_codes,
                                                 const unsigned long long * tipmap, unsigned N, unsigned nblk,
                                                 unsigned R, AncOut out)
{
  extern __shared__ double anc_lds[];
  anc_blocked_body<5>(mv, fidx, node, other, pmat, lut, lut_codes, tipmap, N, nblk, R, out, anc_lds);
}

template <unsigned KS>
__global__ __launch_bounds__(256) void k_anc_s16(ModelView mv, ParamIdx fidx, NodeRef node, NodeRef other,
                                                 const double * pmat, const double * lut, unsigned lut_codes,
                                                 const unsigned long long * tipmap, unsigned N, unsigned nblk,
                                                 unsigned R, AncOut out)
{
  extern __shared__ double anc_lds[];
  anc_blocked_body<KS>(mv, fidx, node, other, pmat, lut, lut_codes, tipmap, N, nblk, R, out, anc_lds);
}

// 4 states, API layout [site][rate][4]; P-matrices [r][4][4], lookup tables [r][code][4]
__global__ __launch_bounds__(256) void k_anc_s4(ModelView mv, ParamIdx fidx, NodeRef node, NodeRef other,
                                                const double * pmat, const double * lut, unsigned lut_codes,
                                                const unsigned long long * tipmap, unsigned N, unsigned R,
                                                AncOut out)
{
  for (unsigned long long n = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; n < N;
       n += (unsigned long long)gridDim.x * blockDim.x)
  {
    const unsigned oc = other.codes ? other.codes[n] : 0u;
    const d4 tipv = node.codes ? tip_value4(tipmap[node.codes[n]]) : d4{0, 0, 0, 0};
    d4 a = {0, 0, 0, 0};
    for (unsigned r = 0; r < R; ++r)
    {
      const double * pi = mv.freqs(fidx.v[r]);
      const double w = mv.weights()[r];
      const double * P = pmat + r * 16;
      d4 t;
      if (other.codes) t = load4(lut + ((size_t)r * lut_codes + oc) * 4);
      else
      {
        const d4 c = load4(other.clv + (n * R + r) * 4);
        t = d4{dot4(P, c), dot4(P + 4, c), dot4(P + 8, c), dot4(P + 12, c)};
      }
      const d4 pv = node.codes ? tipv : load4(node.clv + (n * R + r) * 4);
      a.x += w * pi[0] * pv.x * t.x;
      a.y += w * pi[1] * pv.y * t.y;
      a.z += w * pi[2] * pv.z * t.z;
      a.w += w * pi[3] * pv.w * t.w;
    }
    const double sum = a.x + a.y + a.z + a.w;
    if (sum > 0.0) { a.x /= sum; a.y /= sum; a.z /= sum; a.w /= sum; }
    double best = a.x;
    unsigned idx = 0;
    if (a.y > best) { best = a.y; idx = 1; }
    if (a.z > best) { best = a.z; idx = 2; }
    if (a.w > best) { best = a.w; idx = 3; }
    out.states[n] = (uint8_t)idx;
    out.state_probs[n] = best;
    if (out.probs) store4(out.probs + n * 4, a);
  }
}

// every other family: the arithmetic of k_node_ancestral (kernels_generic.hpp) into the batch's table
__global__ __launch_bounds__(256) void k_anc_generic(ModelView mv, ParamIdx fidx, NodeRef node, NodeRef other,
                                                     const double * pmat, const unsigned long long * tipmap,
                                                     unsigned brows, unsigned N, unsigned R, double * probs)
{
  const unsigned S = mv.S, Sp = mv.Sp;
  for (unsigned long long n = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; n < N;
       n += (unsigned long long)gridDim.x * blockDim.x)
  {
    double * o = probs + n * S;
    double sum = 0.0;
    for (unsigned i = 0; i < S; ++i)
    {
      double v = 0.0;
      for (unsigned r = 0; r < R; ++r)
      {
        const double * row = pmat + ((size_t)r * S + i) * Sp;
        double a = 0.0;
        for (unsigned j = 0; j < S; ++j) a += row[j] * clv_elem(other, tipmap, brows, n, r, j, R, Sp);
        v += mv.weights()[r] * mv.freqs(fidx.v[r])[i] * clv_elem(node, tipmap, brows, n, r, i, R, Sp) * a;
      }
      o[i] = v;
      sum += v;
    }
    if (sum > 0.0)
      for (unsigned i = 0; i < S; ++i) o[i] /= sum;
  }
}

// the summary of a finished table: first index of the row maximum, and the maximum
__global__ __launch_bounds__(256) void k_anc_summary(const double * probs, unsigned N, unsigned S, uint8_t * states,
                                                     double * state_probs)
{
  for (unsigned long long n = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; n < N;
       n += (unsigned long long)gridDim.x * blockDim.x)
  {
    const double * o = probs + n * S;
    double best = o[0];
    unsigned idx = 0;
    for (unsigned i = 1; i < S; ++i)
      if (o[i] > best) { best = o[i]; idx = i; }
    states[n] = (uint8_t)idx;
    state_probs[n] = best;
  }
}

}   // namespace pllhip
