// kernels_sitecat.hpp -- the per-site, per-rate-category likelihood table of an edge (pllhip_sitecat_edge; contract:
// INTEGRATION.md, "Site categories"; design: DESIGN.md section 30).
//
// Value per site n and rate r -- the product the edge kernels form, reduced over STATES and kept per rate:
//     l[n][r] = sum_i pi_r[i] parent[n, r, i] * sum_j P_r[i][j] child[n, r, j]
// with the scaling and p-inv rules of k_edge_lnl_*: c[n] = the scaler counts of both ends (the smallest over the rates
// with PLL_ATTRIB_RATE_SCALERS, the other rates brought down by rate_factor), and the case split of site_loglh -- a
// site with an invariant term and c[n] > 0 has l brought to scale (c <= 3) or dropped, and c[n] = 0.  Out go
//     A[r][n] = (1 - q_r) l[n][r],    B[r][n] = q_r pi_r[invariant[n]]  (only when some q_r > 0),    c[n]
// RATE-major: the posterior and reduction kernels (kernels_sitecat_sums.hpp) read whole planes coalesced, and a blocked
// wave stores one double2 per lane and plane.  Padding sites of the last block are never written.
//
//   k_sitecat_s20 / k_sitecat_s16   blocked families, one body (as anc_blocked_body): a wave owns a 32-site block and
//                                   walks its rates; P_r * child on the matrix cores with the family's addressing, a
//                                   coded child through the matrix's lookup table, a coded parent through the tip map;
//                                   per rate the lane's state rows are added, then the four q lane groups (s20_sum_q).
//   k_sitecat_s4                    API layout, one lane per (site, rate): a wave reads its vectors in one piece.
//   k_sitecat_generic               every other family (33 .. 64 states in blocked rows, the generic API layout): the
//                                   arithmetic of k_edge_lnl_generic through clv_elem.
#pragma once

#include "kernels_common.hpp"
#include "kernels_generic.hpp"
#include "kernels_s4.hpp"
#include "kernels_s20.hpp"
#include "kernels_s16.hpp"

namespace pllhip {

struct SiteCatOut
{
  double * A;          // [R][plane]
  double * B;          // [R][plane] or null (no rate has an invariant part)
  unsigned * c;        // [N] or null (a pass that wants the A planes alone)
  size_t plane;        // doubles between the planes of two rates: even, so that an even site is 16-byte aligned
};

// the two scaler buffers, the invariant states and whether the counts are per rate
struct SiteCatSide
{
  const unsigned * ps, * cs;
  const int * invariant;
  unsigned rate_scalers;
};

// sum_r w_r q_r pi_r[state]: what decides the case split of site_loglh
__device__ inline double sitecat_inv_sum(const ModelView & mv, const ParamIdx & fidx, int state, unsigned R)
{
  double s = 0.0;
  if (state < 0) return s;
  for (unsigned r = 0; r < R; ++r)
  {
    const unsigned fi = fidx.v[r];
    const double q = mv.pinv()[fi];
    if (q > 0.0) s += mv.weights()[r] * q * mv.freqs(fi)[state];
  }
  return s;
}

// l of one (site, rate) -> its rate part and invariant part
__device__ inline void sitecat_entry(const ModelView & mv, unsigned fi, double l, unsigned cnt, bool descale, int state,
                                     double & a, double & b)
{
  if (descale) l = (cnt <= 3) ? ldexp(l, -256 * (int)cnt) : 0.0;
  const double q = mv.pinv()[fi];
  a = (q > 0.0) ? (1.0 - q) * l : l;
  b = (q > 0.0 && state >= 0) ? q * mv.freqs(fi)[state] : 0.0;
}

template <unsigned KS>
__device__ inline void sitecat_blocked_body(const ModelView & mv, const ParamIdx & fidx, const NodeRef & parent,
                                            const NodeRef & child, const double * pmat, const double * lut,
                                            unsigned lut_codes, const unsigned long long * tipmap,
                                            const SiteCatSide & sd, unsigned N, unsigned nblk, unsigned R,
                                            const SiteCatOut & out, double * frag)
{
  constexpr unsigned UNIT = 4 * KS * S20_BS;
  const unsigned S = mv.S;
  if (!child.codes) s16_fill_frags<KS>(frag, pmat, R, S, mv.Sp);
  __syncthreads();

  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned q = lane >> 4, n = lane & 15;
  const unsigned wstride = gridDim.x * 4;

  for (unsigned blk = blockIdx.x * 4 + wave; blk < nblk; blk += wstride)
  {
    const size_t site0 = (size_t)blk * S20_BS + 2 * n;
    const bool live_e = site0 < N, live_o = site0 + 1 < N;
    // (per-site arrays are padded to whole blocks, the padding is zero: every lane reads its two sites)
    unsigned cnt_e, cnt_o;
    if (sd.rate_scalers)
    {
      cnt_e = rate_min_count(sd.ps, sd.cs, site0, R);
      cnt_o = rate_min_count(sd.ps, sd.cs, site0 + 1, R);
    }
    else
    {
      cnt_e = (sd.ps ? sd.ps[site0] : 0u) + (sd.cs ? sd.cs[site0] : 0u);
      cnt_o = (sd.ps ? sd.ps[site0 + 1] : 0u) + (sd.cs ? sd.cs[site0 + 1] : 0u);
    }
    int inv_e = -1, inv_o = -1;
    if (sd.invariant)
    {
      if (live_e) inv_e = sd.invariant[site0];
      if (live_o) inv_o = sd.invariant[site0 + 1];
    }
    const bool desc_e = cnt_e > 0 && sitecat_inv_sum(mv, fidx, inv_e, R) > 0.0;
    const bool desc_o = cnt_o > 0 && sitecat_inv_sum(mv, fidx, inv_o, R) > 0.0;
    unsigned cce = 0, cco = 0;
    unsigned long long pme = 0, pmo = 0;
    if (child.codes) { cce = child.codes[site0]; cco = child.codes[site0 + 1]; }
    if (parent.codes) { pme = tipmap[parent.codes[site0]]; pmo = tipmap[parent.codes[site0 + 1]]; }
    for (unsigned r = 0; r < R; ++r)
    {
      const size_t ubase = ((size_t)blk * R + r) * UNIT;
      const unsigned fi = fidx.v[r];
      const double * pi = mv.freqs(fi);
      double2 t[KS], pv[KS];
      if (child.codes) s16_child_tip<KS>(lut + (size_t)r * lut_codes * S, cce, cco, q, S, t);
      else s16_child_inner<KS>(child.clv + ubase, frag + r * s16_fr(KS), lane, t);
      if (parent.codes) s16_tip_d<KS>(pme, pmo, q, S, pv);
      else s16_load_d<KS>(parent.clv + ubase, lane, pv);
      double le = 0.0, lo = 0.0;
#pragma unroll
      for (unsigned v = 0; v < KS; ++v)
      {
        const unsigned i = 4 * v + q;
        const double f = (i < S) ? pi[i] : 0.0;
        le += f * pv[v].x * t[v].x;
        lo += f * pv[v].y * t[v].y;
      }
      le = s20_sum_q(le);
      lo = s20_sum_q(lo);
      if (sd.rate_scalers)
      {
        le *= rate_factor(sd.ps, sd.cs, site0, R, r, cnt_e);
        lo *= rate_factor(sd.ps, sd.cs, site0 + 1, R, r, cnt_o);
      }
      if (q == 0 && live_e)
      {
        double ae, be, ao = 0.0, bo = 0.0;
        sitecat_entry(mv, fi, le, cnt_e, desc_e, inv_e, ae, be);
        if (live_o) sitecat_entry(mv, fi, lo, cnt_o, desc_o, inv_o, ao, bo);
        const size_t x = (size_t)r * out.plane + site0;
        if (live_o)
        {
          // (site0 is even and the planes start 16-byte aligned: one 16-byte store per lane and plane)
          *reinterpret_cast<double2 *>(out.A + x) = make_double2(ae, ao);
          if (out.B) *reinterpret_cast<double2 *>(out.B + x) = make_double2(be, bo);
        }
        else
        {
          out.A[x] = ae;
          if (out.B) out.B[x] = be;
        }
      }
    }
    if (q == 0 && live_e && out.c)
    {
      out.c[site0] = desc_e ? 0u : cnt_e;
      if (live_o) out.c[site0 + 1] = desc_o ? 0u : cnt_o;
    }
  }
}

// grid = min(ceil(nblk / 4), a few per CU), block = 256; dynamic LDS = R * s16_fr(KS) doubles
__global__ __launch_bounds__(256) void k_sitecat_s20(ModelView mv, ParamIdx fidx, NodeRef parent, NodeRef child,
                                                     const double * pmat, const double * lut, unsigned lut_codes,
                                                     const unsigned long long * tipmap, SiteCatSide sd, unsigned N,
                                                     unsigned nblk, unsigned R, SiteCatOut out)
{
  extern __shared__ double sitecat_lds[];
  sitecat_blocked_body<5>(mv, fidx, parent, child, pmat, lut, lut_codes, tipmap, sd, N, nblk, R, out, sitecat_lds);
}

template <unsigned KS>
__global__ __launch_bounds__(256) void k_sitecat_s16(ModelView mv, ParamIdx fidx, NodeRef parent, NodeRef child,
                                                     const double * pmat, const double * lut, unsigned lut_codes,
                                                     const unsigned long long * tipmap, SiteCatSide sd, unsigned N,
                                                     unsigned nblk, unsigned R, SiteCatOut out)
{
  extern __shared__ double sitecat_lds[];
  sitecat_blocked_body<KS>(mv, fidx, parent, child, pmat, lut, lut_codes, tipmap, sd, N, nblk, R, out, sitecat_lds);
}

// what a thread-per-site kernel does around its l[r]: counts and case split first, then one entry per rate
struct SiteCatSite
{
  unsigned cnt;
  int state;
  bool descale;
};

__device__ inline SiteCatSite sitecat_site(const ModelView & mv, const ParamIdx & fidx, const SiteCatSide & sd,
                                           unsigned long long n, unsigned R)
{
  SiteCatSite st;
  st.cnt = sd.rate_scalers ? rate_min_count(sd.ps, sd.cs, n, R) : (sd.ps ? sd.ps[n] : 0u) + (sd.cs ? sd.cs[n] : 0u);
  st.state = sd.invariant ? sd.invariant[n] : -1;
  st.descale = st.cnt > 0 && sitecat_inv_sum(mv, fidx, st.state, R) > 0.0;
  return st;
}

__device__ inline void sitecat_store(const ModelView & mv, const ParamIdx & fidx, const SiteCatSide & sd,
                                     const SiteCatSite & st, unsigned long long n, unsigned R, unsigned r, double l,
                                     const SiteCatOut & out)
{
  if (sd.rate_scalers) l *= rate_factor(sd.ps, sd.cs, n, R, r, st.cnt);
  double a, b;
  sitecat_entry(mv, fidx.v[r], l, st.cnt, st.descale, st.state, a, b);
  out.A[(size_t)r * out.plane + n] = a;
  if (out.B) out.B[(size_t)r * out.plane + n] = b;
}

// 4 states, API layout [site][rate][4]; P-matrices [r][4][4], lookup tables [r][code][4]
__global__ __launch_bounds__(256) void k_sitecat_s4(ModelView mv, ParamIdx fidx, NodeRef parent, NodeRef child,
                                                    const double * pmat, const double * lut, unsigned lut_codes,
                                                    const unsigned long long * tipmap, SiteCatSide sd, unsigned N,
                                                    unsigned R, SiteCatOut out)
{
  // one lane per (site, rate), as k_edge_lnl_s4 walks them: the lanes of a wave read 2 KiB of a vector in one piece
  // (a thread per site would read its rates 128 bytes apart); the R lanes of a site each make its case split
  const unsigned long long total = (unsigned long long)N * R;
  for (unsigned long long x = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; x < total;
       x += (unsigned long long)gridDim.x * blockDim.x)
  {
    const unsigned long long n = x / R;
    const unsigned r = (unsigned)(x - n * R);
    const SiteCatSite st = sitecat_site(mv, fidx, sd, n, R);
    const double * pi = mv.freqs(fidx.v[r]);
    const double * P = pmat + r * 16;
    d4 t;
    if (child.codes) t = load4(lut + ((size_t)r * lut_codes + child.codes[n]) * 4);
    else
    {
      const d4 c = load4(child.clv + x * 4);
      t = d4{dot4(P, c), dot4(P + 4, c), dot4(P + 8, c), dot4(P + 12, c)};
    }
    const d4 pv = parent.codes ? tip_value4(tipmap[parent.codes[n]]) : load4(parent.clv + x * 4);
    const double l = (pi[0] * pv.x * t.x + pi[1] * pv.y * t.y) + (pi[2] * pv.z * t.z + pi[3] * pv.w * t.w);
    sitecat_store(mv, fidx, sd, st, n, R, r, l, out);
    if (r == 0 && out.c) out.c[n] = st.descale ? 0u : st.cnt;
  }
}

// every other family: the arithmetic of k_edge_lnl_generic, on the API layout (brows = 0) or on blocked rows
__global__ __launch_bounds__(256) void k_sitecat_generic(ModelView mv, ParamIdx fidx, NodeRef parent, NodeRef child,
                                                         const double * pmat, const double * lut, unsigned lut_codes,
                                                         const unsigned long long * tipmap, unsigned brows,
                                                         SiteCatSide sd, unsigned N, unsigned R, SiteCatOut out)
{
  const unsigned S = mv.S, Sp = mv.Sp;
  for (unsigned long long n = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; n < N;
       n += (unsigned long long)gridDim.x * blockDim.x)
  {
    const SiteCatSite st = sitecat_site(mv, fidx, sd, n, R);
    for (unsigned r = 0; r < R; ++r)
    {
      const double * pi = mv.freqs(fidx.v[r]);
      double l = 0.0;
      for (unsigned i = 0; i < S; ++i)
      {
        double a;
        if (child.codes) a = lut[((size_t)r * lut_codes + child.codes[n]) * S + i];
        else
        {
          const double * row = pmat + ((size_t)r * S + i) * Sp;
          a = 0.0;
          for (unsigned j = 0; j < S; ++j) a += row[j] * clv_elem(child, tipmap, brows, n, r, j, R, Sp);
        }
        l += pi[i] * clv_elem(parent, tipmap, brows, n, r, i, R, Sp) * a;
      }
      sitecat_store(mv, fidx, sd, st, n, R, r, l, out);
    }
    if (out.c) out.c[n] = st.descale ? 0u : st.cnt;
  }
}

}   // namespace pllhip
