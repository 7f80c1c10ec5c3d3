// kernels_distance.hpp -- pairwise state-pair counts, distances and neighbour joining (pll_distance_dev.hip; contract:
// INTEGRATION.md, "Pairwise distances and neighbour joining"; design: DESIGN.md section 23).
//
//   k_dst_codes<CODED>   one byte per (taxon, staged column): the state of a character whose mask has exactly one bit,
//       DST_NONE otherwise.  A staged column is a site with a weight of 1 .. 127; the host splits heavier sites.
//   k_dst_counts         N = X diag(w) X^T with v_mfma_i32_16x16x64_i8, X the 0/1 matrix with one row per
//       (taxon, state) and one column per staged column.  A wave owns a 64 x 64 tile of N (4 x 4 MFMA tiles) over one
//       range of columns: per 64 columns it builds four weighted and four plain one-hot fragments from 16 code bytes
//       per lane (byte-parallel compares, no branch) and issues sixteen MFMAs.  Lane l holds row (l & 15) and the 16
//       columns of group (l >> 4) in both operands -- both built by dst_onehot, so the order of the columns inside an
//       instruction cannot matter -- and element v of the result is row 4 (l >> 4) + v, column (l & 15).  Only tiles
//       that reach the diagonal or lie above it are made.  What is not zero is added with integer atomics: exact, and
//       the same whatever the order.
//   k_dst_estimate       one wave per taxon pair: n and the trace from the S x S block, then p, JC or the ML distance
//       by bracketed Newton steps on lnL'(t) with analytic derivatives from the eigen-decomposition.
//   k_nj_*               neighbour joining, two launches per round: the arg-min of Q over (value, i, j) keys per
//       workgroup, then one workgroup that picks the join, writes its record and updates the row of the new node.
//       No kernel waits for another workgroup.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "tip_view.hpp"

namespace pllhip {

constexpr unsigned DST_WG = 256;
constexpr uint8_t DST_NONE = 0xFF;
constexpr unsigned DST_TILE = 64;            // rows and columns of a wave's tile
constexpr int DST_FR = DST_TILE / 16;        // MFMA tiles along each side of it
constexpr unsigned DST_KSTEP = 64;           // columns per MFMA
constexpr unsigned DST_MAX_W = 127;          // weight of a staged column (a positive int8)
constexpr unsigned DST_MAX_STATES = 64;
// status words of k_dst_codes
constexpr unsigned DST_BAD = 0;              // min over unmapped characters of tip * sites + site (DST_NO_BAD: none)
constexpr unsigned DST_NONBIN = 1;           // != 0: a tip vector holds an entry that is neither 0 nor 1
constexpr unsigned long long DST_NO_BAD = ~0ULL;
constexpr unsigned NJ_MAX_GRID = 256;

using dst_v4i = __attribute__((ext_vector_type(4))) int;

template <bool CODED>
__global__ __launch_bounds__(DST_WG) void k_dst_codes(TipView tp, const unsigned long long * __restrict__ tipmap,
                                                      const unsigned * __restrict__ col_site, unsigned T, unsigned N,
                                                      unsigned S, unsigned C, unsigned long long Cpad,
                                                      uint8_t * __restrict__ codes,
                                                      unsigned long long * __restrict__ status)
{
  const unsigned long long c = (unsigned long long)blockIdx.x * DST_WG + threadIdx.x;
  if (c >= Cpad) return;
  const unsigned long long full = S < 64 ? ((1ULL << S) - 1ULL) : ~0ULL;
  const unsigned n = c < C ? col_site[c] : 0u;
  for (unsigned t = blockIdx.y; t < T; t += gridDim.y)
  {
    uint8_t code = DST_NONE;
    if (c < C)
    {
      if (CODED)
      {
        const uint8_t * row = tp.code_rows ? tp.code_rows[t] : tp.code_base + (unsigned long long)t * tp.code_stride;
        const unsigned long long raw = tipmap[row[n]];
        if (!raw) atomicMin(status + DST_BAD, (unsigned long long)t * N + n);
        const unsigned long long m = raw & full;
        if (__popcll(m) == 1) code = (uint8_t)__builtin_ctzll(m);
      }
      else
      {
        unsigned ones = 0, which = 0;
        bool other = false;
        for (unsigned k = 0; k < S; ++k)
        {
          const double x = tip_clv(tp, t, n, k);
          if (x == 1.0) { ++ones; which = k; }
          else if (x != 0.0) other = true;
        }
        if (other) status[DST_NONBIN] = 1;                 // (every writer stores the same value)
        if (ones == 1) code = (uint8_t)which;
      }
    }
    codes[(unsigned long long)t * Cpad + c] = code;
  }
}

// four code bytes against a state in every byte: 1 in the bytes that are equal, 0 in the others
__device__ inline unsigned dst_onehot(unsigned word, unsigned state4)
{
  const unsigned x = word ^ state4;
  const unsigned t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  return (~(t | x | 0x7F7F7F7Fu)) >> 7;
}

__device__ inline dst_v4i dst_plain(uint4 c, unsigned s4)
{
  dst_v4i f;
  f[0] = (int)dst_onehot(c.x, s4); f[1] = (int)dst_onehot(c.y, s4);
  f[2] = (int)dst_onehot(c.z, s4); f[3] = (int)dst_onehot(c.w, s4);
  return f;
}

__device__ inline dst_v4i dst_weighted(uint4 c, unsigned s4, uint4 w)
{
  dst_v4i f;
  f[0] = (int)(w.x & (dst_onehot(c.x, s4) * 0xFFu)); f[1] = (int)(w.y & (dst_onehot(c.y, s4) * 0xFFu));
  f[2] = (int)(w.z & (dst_onehot(c.z, s4) * 0xFFu)); f[3] = (int)(w.w & (dst_onehot(c.w, s4) * 0xFFu));
  return f;
}

// out[band_rows][M] += the band's rows of N.  Row r of the band is row row0 + r of N; rows and columns are
// taxon * S + state.  grid = (column tiles, row tiles, column ranges of `chunk`), one wave each.
__global__ __launch_bounds__(64) void k_dst_counts(const uint8_t * __restrict__ codes, const uint8_t * __restrict__ wq,
                                                   unsigned long long Cpad, unsigned S, unsigned row0,
                                                   unsigned band_rows, unsigned M, unsigned long long chunk,
                                                   int * __restrict__ out)
{
  const unsigned cj = blockIdx.x, ri = blockIdx.y;
  if ((unsigned long long)cj * DST_TILE + (DST_TILE - 1) < (unsigned long long)row0 + ri * DST_TILE) return;   // below
  const unsigned lane = threadIdx.x, r = lane & 15u, g = lane >> 4;
  const unsigned long long kbeg = (unsigned long long)blockIdx.z * chunk;
  const unsigned long long kend = kbeg + chunk < Cpad ? kbeg + chunk : Cpad;

  // a row or column past the end compares against a state no code has
  const uint8_t * pa[DST_FR], * pb[DST_FR];
  unsigned sa[DST_FR], sb[DST_FR];
#pragma unroll
  for (int m = 0; m < DST_FR; ++m)
  {
    const unsigned lr = ri * DST_TILE + m * 16 + r, gr = row0 + lr;
    const bool ok = lr < band_rows;
    pa[m] = codes + (ok ? (unsigned long long)(gr / S) * Cpad : 0ULL) + g * 16;
    sa[m] = (ok ? gr % S : 0xFEu) * 0x01010101u;
    const unsigned gc = cj * DST_TILE + m * 16 + r;
    const bool okc = gc < M;
    pb[m] = codes + (okc ? (unsigned long long)(gc / S) * Cpad : 0ULL) + g * 16;
    sb[m] = (okc ? gc % S : 0xFEu) * 0x01010101u;
  }
  dst_v4i acc[DST_FR][DST_FR];
#pragma unroll
  for (int m = 0; m < DST_FR; ++m)
#pragma unroll
    for (int n = 0; n < DST_FR; ++n) acc[m][n] = dst_v4i{0, 0, 0, 0};

  for (unsigned long long k = kbeg; k < kend; k += DST_KSTEP)
  {
    const uint4 w = *reinterpret_cast<const uint4 *>(wq + k + g * 16);
    dst_v4i fa[DST_FR], fb[DST_FR];
#pragma unroll
    for (int m = 0; m < DST_FR; ++m)
    {
      fa[m] = dst_weighted(*reinterpret_cast<const uint4 *>(pa[m] + k), sa[m], w);
      fb[m] = dst_plain(*reinterpret_cast<const uint4 *>(pb[m] + k), sb[m]);
    }
#pragma unroll
    for (int m = 0; m < DST_FR; ++m)
#pragma unroll
      for (int n = 0; n < DST_FR; ++n)
        acc[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m], fb[n], acc[m][n], 0, 0, 0);
  }

#pragma unroll
  for (int m = 0; m < DST_FR; ++m)
#pragma unroll
    for (int n = 0; n < DST_FR; ++n)
#pragma unroll
      for (int v = 0; v < 4; ++v)
      {
        const unsigned lr = ri * DST_TILE + m * 16 + 4 * g + v, gc = cj * DST_TILE + n * 16 + r;
        if (acc[m][n][v] && lr < band_rows && gc < M) atomicAdd(out + (unsigned long long)lr * M + gc, acc[m][n][v]);
      }
}

// the model of the ML distance: P(t) = V exp(L c_r t) V^-1, parameter set 0
struct DstModel
{
  const double * V;        // [S][Sp]   (partition->inv_eigenvecs)
  const double * Vi;       // [S][Sp]   (partition->eigenvecs)
  const double * evals;    // [Sp]
  const double * rates;    // [R]
  const double * rate_w;   // [R]
  unsigned R, Sp;
  double pinv;
};

__device__ inline double dst_wave_sum(double v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ inline long long dst_wave_sum(long long v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// lnL'(t) and lnL''(t) of one pair; every lane returns the same bits (a butterfly of commutative additions)
__device__ inline void dst_derivatives(const int * __restrict__ blk, unsigned M, unsigned S, const DstModel & md, double t,
                                       double * sG, double & d1, double & d2)
{
  const unsigned lane = threadIdx.x;
  __syncthreads();
  for (unsigned k = lane; k < S; k += 64)
  {
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (unsigned r = 0; r < md.R; ++r)
    {
      const double c = md.evals[k] * (md.rates[r] / (1.0 - md.pinv));
      const double e = md.rate_w[r] * exp(c * t);
      g0 += e;
      g1 += c * e;
      g2 += c * c * e;
    }
    sG[k] = g0; sG[DST_MAX_STATES + k] = g1; sG[2 * DST_MAX_STATES + k] = g2;
  }
  __syncthreads();
  double s1 = 0.0, s2 = 0.0;
  for (unsigned e = lane; e < S * S; e += 64)
  {
    const unsigned a = e / S, b = e % S;
    const int cnt = blk[(unsigned long long)a * M + b];
    if (!cnt) continue;
    double f = 0.0, f1 = 0.0, f2 = 0.0;
    for (unsigned k = 0; k < S; ++k)
    {
      const double vv = md.V[a * md.Sp + k] * md.Vi[k * md.Sp + b];
      f += vv * sG[k];
      f1 += vv * sG[DST_MAX_STATES + k];
      f2 += vv * sG[2 * DST_MAX_STATES + k];
    }
    const double q = 1.0 - md.pinv;
    f = q * f + (a == b ? md.pinv : 0.0);
    f1 *= q;
    f2 *= q;
    if (!(f > 1e-300)) f = 1e-300;
    const double u = f1 / f;
    s1 += (double)cnt * u;
    s2 += (double)cnt * (f2 / f - u * u);
  }
  d1 = dst_wave_sum(s1);
  d2 = dst_wave_sum(s2);
}

// grid = (T, taxa of the band), one wave each; counts[band taxa * S][M]
__global__ __launch_bounds__(64) void k_dst_estimate(const int * __restrict__ counts, unsigned t0, unsigned M, unsigned S,
                                                     unsigned T, DstModel md, int method, double dmin, double dmax,
                                                     double * __restrict__ D, unsigned * __restrict__ compared,
                                                     unsigned long long * __restrict__ no_overlap)
{
#pragma clang fp contract(off)
  __shared__ double sG[3 * DST_MAX_STATES];
  const unsigned i = t0 + blockIdx.y, j = blockIdx.x, lane = threadIdx.x;
  if (j < i) return;
  const int * blk = counts + (unsigned long long)(blockIdx.y * S) * M + (unsigned long long)j * S;
  long long n = 0, tr = 0;
  for (unsigned e = lane; e < S * S; e += 64)
  {
    const unsigned a = e / S, b = e % S;
    const int cnt = blk[(unsigned long long)a * M + b];
    n += cnt;
    if (a == b) tr += cnt;
  }
  n = dst_wave_sum(n);
  tr = dst_wave_sum(tr);
  double d = 0.0;
  if (i != j)
  {
    if (n == 0)
    {
      d = dmax;
      if (lane == 0) atomicAdd(no_overlap, 1ULL);
    }
    else if (method == 0) d = (double)(n - tr) / (double)n;
    else if (method == 1)
    {
      const double p = (double)(n - tr) / (double)n, b = (double)(S - 1) / (double)S;
      d = p >= b ? dmax : -b * log(1.0 - p / b);
    }
    else
    {
      double d1, d2, lo = dmin, hi = dmax;
      dst_derivatives(blk, M, S, md, lo, sG, d1, d2);
      if (d1 <= 0.0) d = dmin;
      else
      {
        dst_derivatives(blk, M, S, md, hi, sG, d1, d2);
        if (d1 >= 0.0) d = dmax;
        else
        {
          // start at the JC distance where it lies inside the bracket
          const double p = (double)(n - tr) / (double)n, b = (double)(S - 1) / (double)S;
          double t = p < b ? -b * log(1.0 - p / b) : 1.0;
          if (!(t > lo && t < hi)) t = 0.5 * (lo + hi);
          for (int it = 0; it < 200; ++it)
          {
            dst_derivatives(blk, M, S, md, t, sG, d1, d2);
            if (d1 == 0.0) break;
            if (d1 > 0.0) lo = t; else hi = t;
            double next = d2 < 0.0 ? t - d1 / d2 : hi;          // (hi: rejected below)
            if (!(next > lo && next < hi)) next = 0.5 * (lo + hi);
            const double step = fabs(next - t);
            t = next;
            if (step <= 1e-14 * t || hi - lo <= 1e-14 * hi) break;
          }
          d = t;
        }
      }
    }
  }
  if (lane == 0)
  {
    D[(unsigned long long)i * T + j] = d;
    D[(unsigned long long)j * T + i] = d;
    compared[(unsigned long long)i * T + j] = (unsigned)n;
    compared[(unsigned long long)j * T + i] = (unsigned)n;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// neighbour joining
// ---------------------------------------------------------------------------------------------------------------------
struct NjKey
{
  double q;
  unsigned i, j;
};

__device__ inline bool nj_less(const NjKey & a, const NjKey & b)
{
  return a.q < b.q || (a.q == b.q && (a.i < b.i || (a.i == b.i && a.j < b.j)));
}

// the smallest key of the workgroup in every lane of thread 0's wave (sKey: DST_WG entries)
__device__ inline NjKey nj_block_min(NjKey best, NjKey * sKey)
{
  const unsigned tid = threadIdx.x;
  sKey[tid] = best;
  __syncthreads();
  for (unsigned half = DST_WG / 2; half > 0; half >>= 1)
  {
    if (tid < half && nj_less(sKey[tid + half], sKey[tid])) sKey[tid] = sKey[tid + half];
    __syncthreads();
  }
  return sKey[0];
}

// r[i] = d[i][0] + d[i][1] + ... in that order
__global__ __launch_bounds__(DST_WG) void k_nj_rowsum(const double * __restrict__ D, unsigned T, double * __restrict__ r)
{
#pragma clang fp contract(off)
  const unsigned i = blockIdx.x * DST_WG + threadIdx.x;
  if (i >= T) return;
  double s = 0.0;
  for (unsigned k = 0; k < T; ++k) s += D[(unsigned long long)i * T + k];
  r[i] = s;
}

// block_min[block] = the smallest (Q, i, j) among the rows of `alive` this workgroup owns; alive[0 .. n) ascending
__global__ __launch_bounds__(DST_WG) void k_nj_min(const double * __restrict__ D, const double * __restrict__ r,
                                                   const unsigned * __restrict__ alive, unsigned n, unsigned T,
                                                   NjKey * __restrict__ block_min)
{
#pragma clang fp contract(off)
  __shared__ NjKey sKey[DST_WG];
  const double n2 = (double)(n - 2u);
  NjKey best = {INFINITY, ~0u, ~0u};
  for (unsigned a = blockIdx.x; a + 1 < n; a += gridDim.x)
  {
    const unsigned i = alive[a];
    const double ri = r[i];
    for (unsigned b = a + 1 + threadIdx.x; b < n; b += DST_WG)
    {
      const unsigned j = alive[b];
      const double prod = n2 * D[(unsigned long long)i * T + j];
      const double q1 = prod - ri;
      const NjKey key = {q1 - r[j], i, j};
      if (nj_less(key, best)) best = key;
    }
  }
  best = nj_block_min(best, sKey);
  if (threadIdx.x == 0) block_min[blockIdx.x] = best;
}

// one workgroup: the join of this round from the workgroups' minima, its record, the new node's row in slot i,
// slot j leaves `alive`
__global__ __launch_bounds__(DST_WG) void k_nj_join(double * __restrict__ D, double * __restrict__ r,
                                                    unsigned * __restrict__ alive, unsigned n, unsigned T,
                                                    const NjKey * __restrict__ block_min, unsigned blocks, unsigned round,
                                                    unsigned * __restrict__ slots, double * __restrict__ lengths)
{
#pragma clang fp contract(off)
  __shared__ NjKey sKey[DST_WG];
  __shared__ unsigned sPos;
  const unsigned tid = threadIdx.x;
  NjKey best = {INFINITY, ~0u, ~0u};
  for (unsigned b = tid; b < blocks; b += DST_WG)
    if (nj_less(block_min[b], best)) best = block_min[b];
  best = nj_block_min(best, sKey);
  const unsigned i = best.i, j = best.j;
  if (i >= T || j >= T) return;                            // (no finite Q: the host rejects such matrices)
  const double dij = D[(unsigned long long)i * T + j], ri = r[i], rj = r[j];
  const double nd = (double)n;
  __syncthreads();                                         // every lane holds d_ij, r_i, r_j before anything is written
  if (tid == 0)
  {
    const double half = dij / 2.0;
    const double li = half + (ri - rj) / (2.0 * (nd - 2.0));
    slots[2 * round] = i;
    slots[2 * round + 1] = j;
    lengths[2 * round] = li;
    lengths[2 * round + 1] = dij - li;
  }
  for (unsigned a = tid; a < n; a += DST_WG)
  {
    const unsigned k = alive[a];
    if (k == j) sPos = a;
    if (k == i || k == j) continue;
    const double dik = D[(unsigned long long)i * T + k], djk = D[(unsigned long long)j * T + k];
    const double duk = ((dik + djk) - dij) / 2.0;
    r[k] = ((r[k] - dik) - djk) + duk;
    D[(unsigned long long)i * T + k] = duk;
    D[(unsigned long long)k * T + i] = duk;
  }
  if (tid == 0) r[i] = ((ri + rj) - nd * dij) / 2.0;
  __syncthreads();
  // alive[sPos ..] moves down by one, a stretch of DST_WG at a time
  for (unsigned base = sPos; base + 1 < n; base += DST_WG)
  {
    const unsigned a = base + tid;
    const unsigned next = a + 1 < n ? alive[a + 1] : 0u;
    __syncthreads();
    if (a + 1 < n) alive[a] = next;
    __syncthreads();
  }
}

// the last three slots meet in one node
__global__ void k_nj_last(const double * __restrict__ D, const unsigned * __restrict__ alive, unsigned T, unsigned round,
                          unsigned * __restrict__ slots, double * __restrict__ lengths)
{
#pragma clang fp contract(off)
  if (threadIdx.x || blockIdx.x) return;
  const unsigned a = alive[0], b = alive[1], c = alive[2];
  const double dab = D[(unsigned long long)a * T + b], dac = D[(unsigned long long)a * T + c],
               dbc = D[(unsigned long long)b * T + c];
  slots[2 * round] = a; slots[2 * round + 1] = b; slots[2 * round + 2] = c;
  lengths[2 * round] = ((dab + dac) - dbc) / 2.0;
  lengths[2 * round + 1] = ((dab + dbc) - dac) / 2.0;
  lengths[2 * round + 2] = ((dac + dbc) - dab) / 2.0;
}

} // namespace pllhip
