// kernels_substmap.hpp -- the endpoint-pair table of an edge (pllhip_substmap_edge; contract: INTEGRATION.md,
// "Substitution mapping"; design: DESIGN.md section 31).
//
//     F[r][i][j] = pi_r[i] * sum_n (m_n s[n][r]) parent[n, r, i] child[n, r, j]
//
// a matrix product whose K dimension is the sites.  Three steps, all on the partition's stream:
//
//   k_substmap_scale            one thread per site: from the site-category table of the edge (A, B: kernels_sitecat.hpp)
//                               the rate-major plane m_n s[n][r] = m_n w_r (1 - q_r) d[n][r] / T[n], d through the very
//                               functions the table kernels apply it with (sitecat_site, rate_factor, sitecat_entry at
//                               l = 1), and differ[n] = sum_r w_r A0[n][r] / T[n], A0 the table under the matrices with a
//                               zeroed diagonal (k_substmap_zero_diag).  Sites past N (the plane is padded to whole
//                               32-site blocks) get 0.
//   k_substmap_pairs_blocked    s20-mfma and s16-mfma<KS>: v_mfma_f64_16x16x4_f64 over the sites, operands read from the
//                               units as they lie (see there).
//   k_substmap_pairs_generic    every other family: the partial tile of one rate in LDS, elements through clv_elem.
//   k_substmap_reduce           adds the partial tiles of the workgroups in workgroup order: F and pairs = F o P.
//
// No floating-point atomics anywhere: F is a function of the inputs and the grid.
#pragma once

#include "kernels_sitecat.hpp"

namespace pllhip {

// pm0 = pm with a zeroed diagonal, [R][S][Sp]
__global__ __launch_bounds__(256) void k_substmap_zero_diag(const double * pm, double * pm0, unsigned R, unsigned S,
                                                            unsigned Sp)
{
  const unsigned total = R * S * Sp;
  for (unsigned x = blockIdx.x * blockDim.x + threadIdx.x; x < total; x += gridDim.x * blockDim.x)
  {
    const unsigned j = x % Sp, i = (x / Sp) % S;
    pm0[x] = (i == j) ? 0.0 : pm[x];
  }
}

struct SubstScale
{
  const double * A, * B, * A0;     // [R][plane]; B null: no invariant part; A0 null: no differ
  size_t plane;
  const unsigned * m;              // [N] pattern weights
  double * scale;                  // [R][splane]
  size_t splane;                   // a multiple of 32, >= N
  double * differ;                 // [N] or null
  unsigned long long * dropped;    // one counter: sites with m_n > 0 and T = 0
};

__global__ __launch_bounds__(256) void k_substmap_scale(ModelView mv, ParamIdx fidx, SiteCatSide sd, unsigned N, unsigned R,
                                                        SubstScale io)
{
  for (unsigned long long n = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; n < io.splane;
       n += (unsigned long long)gridDim.x * blockDim.x)
  {
    if (n >= N)
    {
      for (unsigned r = 0; r < R; ++r) io.scale[(size_t)r * io.splane + n] = 0.0;
      continue;
    }
    const SiteCatSite st = sitecat_site(mv, fidx, sd, n, R);
    double T = 0.0;
    for (unsigned r = 0; r < R; ++r)
      T += mv.weights()[r] * (io.A[(size_t)r * io.plane + n] + (io.B ? io.B[(size_t)r * io.plane + n] : 0.0));
    const bool live = T > 0.0;
    const unsigned mn = io.m[n];
    double df = 0.0;
    for (unsigned r = 0; r < R; ++r)
    {
      // (1 - q_r) d[n][r]: the table's own treatment of l = 1
      double l = 1.0, a, b;
      if (sd.rate_scalers) l *= rate_factor(sd.ps, sd.cs, n, R, r, st.cnt);
      sitecat_entry(mv, fidx.v[r], l, st.cnt, st.descale, st.state, a, b);
      const double w = mv.weights()[r];
      io.scale[(size_t)r * io.splane + n] = live ? (double)mn * ((w * a) / T) : 0.0;
      if (io.A0 && live) df += (w * io.A0[(size_t)r * io.plane + n]) / T;
    }
    if (io.differ) io.differ[n] = df;
    if (mn && !live) atomicAdd(io.dropped, 1ULL);
  }
}

// Blocked families.  A (block, rate) unit is [4 KS state rows][32 sites], state-major.  The instruction wants, in lane
// 16 q + n, A[i = n][k = q] and B[k = q][j = n] and sums over k; here k is a site, i a parent state, j a child state.
// Which site a (k-step, q) pair stands for is free as long as both operands and the scale agree, so lane (q, n) takes
// the EIGHT CONTIGUOUS sites 8 q .. 8 q + 7 of state row 16 t + n -- two 32-byte loads per row and tile, the four q
// lanes of a row reading its 256 bytes in one piece -- and k-step k multiplies site 8 q + k.  No LDS staging, no
// transpose.  Rows from 4 KS up are zero operands (not read); sites from N up are zeroed in both operands.  A coded
// side builds its operand from the mask bits.  The parent operand carries the scale; pi_r[i] is applied in the
// reduction.  A wave walks the blocks of its share for one rate after the other; the four waves of a workgroup add
// their tiles through LDS in wave order and the workgroup writes one partial tile [S][S] per rate.
template <unsigned KS>
__global__ __launch_bounds__(256) void k_substmap_pairs_blocked(NodeRef parent, NodeRef child,
                                                                const unsigned long long * tipmap, const double * scale,
                                                                size_t splane, unsigned N, unsigned nblk, unsigned R,
                                                                unsigned S, double * partial)
{
  constexpr unsigned MT = (KS + 3) / 4, ROWS = 4 * KS, UNIT = ROWS * S20_BS, TS = 16 * MT;
  __shared__ double red[4][TS * TS];
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned q = lane >> 4, n = lane & 15;
  const unsigned wstride = gridDim.x * 4;
  for (unsigned r = 0; r < R; ++r)
  {
    v4d acc[MT][MT];
#pragma unroll
    for (unsigned ti = 0; ti < MT; ++ti)
#pragma unroll
      for (unsigned tj = 0; tj < MT; ++tj) acc[ti][tj] = v4d{0, 0, 0, 0};
    for (unsigned blk = blockIdx.x * 4 + wave; blk < nblk; blk += wstride)
    {
      const size_t site0 = (size_t)blk * S20_BS + 8 * q;
      const size_t ubase = ((size_t)blk * R + r) * UNIT;
      const double * sp = scale + (size_t)r * splane + site0;
      const v4d s0 = *reinterpret_cast<const v4d *>(sp), s1 = *reinterpret_cast<const v4d *>(sp + 4);
      double sc[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
      bool live[8];
      unsigned long long pmask[8], cmask[8];
#pragma unroll
      for (unsigned k = 0; k < 8; ++k)
      {
        live[k] = site0 + k < N;
        pmask[k] = (parent.codes && live[k]) ? tipmap[parent.codes[site0 + k]] : 0ULL;
        cmask[k] = (child.codes && live[k]) ? tipmap[child.codes[site0 + k]] : 0ULL;
      }
      double a[MT][8], b[MT][8];
#pragma unroll
      for (unsigned t = 0; t < MT; ++t)
      {
        const unsigned row = 16 * t + n;
        if (parent.codes)
        {
#pragma unroll
          for (unsigned k = 0; k < 8; ++k) a[t][k] = (row < S && ((pmask[k] >> row) & 1ULL)) ? sc[k] : 0.0;
        }
        else if (row < ROWS)
        {
          const double * up = parent.clv + ubase + (size_t)row * S20_BS + 8 * q;
          const v4d x0 = *reinterpret_cast<const v4d *>(up), x1 = *reinterpret_cast<const v4d *>(up + 4);
          const double x[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
#pragma unroll
          for (unsigned k = 0; k < 8; ++k) a[t][k] = live[k] ? sc[k] * x[k] : 0.0;
        }
        else
        {
#pragma unroll
          for (unsigned k = 0; k < 8; ++k) a[t][k] = 0.0;
        }
        if (child.codes)
        {
#pragma unroll
          for (unsigned k = 0; k < 8; ++k) b[t][k] = (row < S && ((cmask[k] >> row) & 1ULL)) ? 1.0 : 0.0;
        }
        else if (row < ROWS)
        {
          const double * up = child.clv + ubase + (size_t)row * S20_BS + 8 * q;
          const v4d x0 = *reinterpret_cast<const v4d *>(up), x1 = *reinterpret_cast<const v4d *>(up + 4);
          const double x[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
#pragma unroll
          for (unsigned k = 0; k < 8; ++k) b[t][k] = live[k] ? x[k] : 0.0;
        }
        else
        {
#pragma unroll
          for (unsigned k = 0; k < 8; ++k) b[t][k] = 0.0;
        }
      }
#pragma unroll
      for (unsigned k = 0; k < 8; ++k)
#pragma unroll
        for (unsigned ti = 0; ti < MT; ++ti)
#pragma unroll
          for (unsigned tj = 0; tj < MT; ++tj) acc[ti][tj] = mfma_f64(a[ti][k], b[tj][k], acc[ti][tj]);
    }
    // D register v of lane (q, n): row 4 v + q, column n of its tile
#pragma unroll
    for (unsigned ti = 0; ti < MT; ++ti)
#pragma unroll
      for (unsigned tj = 0; tj < MT; ++tj)
#pragma unroll
        for (unsigned v = 0; v < 4; ++v)
          red[wave][(16 * ti + 4 * v + q) * TS + 16 * tj + n] = acc[ti][tj][v];
    __syncthreads();
    double * out = partial + ((size_t)blockIdx.x * R + r) * S * S;
    for (unsigned e = threadIdx.x; e < S * S; e += 256)
    {
      const unsigned x = (e / S) * TS + e % S;
      out[e] = ((red[0][x] + red[1][x]) + red[2][x]) + red[3][x];
    }
    __syncthreads();
  }
}

// Every other family (4 states; 33 .. 64 states in blocked rows; the API layout): a workgroup takes chunks of CH sites,
// stages scale * parent and child of the chunk in LDS ([site][state]) and adds the chunk to its partial tile, which
// lives in LDS as G slices of [S][S] (G = max(1, 256 / S^2): with few states a slice takes every G-th site of a chunk,
// so that all 256 threads have an entry).  Entry x of the tile belongs to thread x mod 256 alone.  After the last chunk
// of a rate the slices are added in slice order.  dynamic LDS = (G S^2 + 2 CH S) doubles.
__global__ __launch_bounds__(256) void k_substmap_pairs_generic(NodeRef parent, NodeRef child,
                                                                const unsigned long long * tipmap, unsigned brows,
                                                                const double * scale, size_t splane, unsigned N,
                                                                unsigned R, unsigned S, unsigned Sp, unsigned CH,
                                                                unsigned G, double * partial)
{
  extern __shared__ double substmap_lds[];
  const unsigned E = S * S, items = G * E;
  double * tile = substmap_lds, * sa = tile + items, * sb = sa + CH * S;
  const unsigned nchunks = (N + CH - 1) / CH;
  for (unsigned r = 0; r < R; ++r)
  {
    for (unsigned x = threadIdx.x; x < items; x += 256) tile[x] = 0.0;
    for (unsigned c = blockIdx.x; c < nchunks; c += gridDim.x)
    {
      __syncthreads();                                   // (the chunk before has been read)
      const unsigned long long base = (unsigned long long)c * CH;
      const unsigned cnt = (unsigned)(N - base < CH ? N - base : CH);
      for (unsigned x = threadIdx.x; x < cnt * S; x += 256)
      {
        const unsigned nl = x / S, j = x % S;
        const unsigned long long site = base + nl;
        sa[x] = scale[(size_t)r * splane + site] * clv_elem(parent, tipmap, brows, site, r, j, R, Sp);
        sb[x] = clv_elem(child, tipmap, brows, site, r, j, R, Sp);
      }
      __syncthreads();
      for (unsigned x = threadIdx.x; x < items; x += 256)
      {
        const unsigned g = x / E, e = x % E, i = e / S, j = e % S;
        double acc = tile[x];
        for (unsigned nl = g; nl < cnt; nl += G) acc += sa[nl * S + i] * sb[nl * S + j];
        tile[x] = acc;
      }
    }
    __syncthreads();
    double * out = partial + ((size_t)blockIdx.x * R + r) * E;
    for (unsigned e = threadIdx.x; e < E; e += 256)
    {
      double sum = tile[e];
      for (unsigned g = 1; g < G; ++g) sum += tile[g * E + e];
      out[e] = sum;
    }
    __syncthreads();
  }
}

// F[r][i][j] = pi_r[i] * (partial tiles added in workgroup order), pairs = F o P_r.  A workgroup takes 64 consecutive
// entries of [R][S][S]; its four waves add every fourth tile each (coalesced rows of 512 bytes) and thread 0 .. 63 adds
// the four sums in wave order.
__global__ __launch_bounds__(256) void k_substmap_reduce(const double * partial, unsigned nparts, unsigned R, unsigned S,
                                                         unsigned Sp, const double * pmat, ModelView mv, ParamIdx fidx,
                                                         double * F, double * pairs)
{
  __shared__ double part[4][64];
  const unsigned E = S * S, total = R * E;
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned x = blockIdx.x * 64 + lane;
  double sum = 0.0;
  if (x < total)
    for (unsigned b = wave; b < nparts; b += 4) sum += partial[(size_t)b * total + x];
  part[wave][lane] = sum;
  __syncthreads();
  if (wave == 0 && x < total)
  {
    const unsigned r = x / E, e = x % E, i = e / S, j = e % S;
    const double f = mv.freqs(fidx.v[r])[i] * (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]);
    F[x] = f;
    pairs[x] = f * pmat[((size_t)r * S + i) * Sp + j];
  }
}

}   // namespace pllhip
