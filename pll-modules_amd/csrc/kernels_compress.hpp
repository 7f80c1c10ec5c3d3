// kernels_compress.hpp -- site-pattern compression of an alignment (pll_compress_site_patterns, pll_compress_dev.hip).
//
// Layout: the alignment is [taxon][Lp] bytes, Lp = the site count rounded up to 256, so that a wave's load of one
// taxon -- 64 lanes x 4 consecutive sites -- is one aligned run of 256 bytes.  Characters are compared through a
// 256-entry table of canonical codes (characters with equal map value share a code; map == 0 is MSA_ILLEGAL); the
// table travels as a kernel argument and sits in LDS.
//
//   k_msa_hash     one pass over the T x L bytes: two independent 64-bit hashes of every column's codes
//   k_msa_insert   open-addressing table {tag | owner site}; a tag match is confirmed by comparing the two columns
//                  in full, so unequal columns never merge whatever the hashes do
//   k_msa_scan_*   patterns numbered by first occurrence: an exclusive prefix sum over "site is the first of its
//                  group", tiles of 4096 as in kernels_repeats.hpp, applied recursively beyond 1024 tiles
//   k_msa_number   pattern index of every site
//   k_msa_gather   out[t][p] = in[t][first site of p]
//
// Which site owns a slot is a race.  Everything that leaves the device is derived from the owner only through
// min(site) (first occurrence) and an integer count (weight), so the results are the same from run to run.
// No per-lane arrays: a lane's state in the hash pass is eight 64-bit hashes.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace pllhip {

constexpr unsigned MSA_WG = 256;
constexpr unsigned MSA_ILLEGAL = 0xffffu;                      // canonical code of a character with map == 0
constexpr unsigned long long MSA_EMPTY = ~0ULL;                // empty slot (a site index never is 0xffffffff)
constexpr unsigned long long MSA_NO_BAD = ~0ULL;
constexpr unsigned MSA_SCAN_TILE = 4096;                       // entries per workgroup of the scan (1024 lanes x 4)

struct MsaCodes
{
  uint16_t code[256];
};

__device__ inline void msa_load_codes(uint16_t * lds, const MsaCodes & codes)
{
  for (unsigned i = threadIdx.x; i < 256u; i += blockDim.x) lds[i] = codes.code[i];
  __syncthreads();
}

__device__ inline unsigned long long msa_fmix(unsigned long long k, unsigned long long m1, unsigned long long m2)
{
  k ^= k >> 33; k *= m1; k ^= k >> 33; k *= m2; k ^= k >> 33;
  return k;
}

// hashes of the columns.  grid = chunks of 1024 sites (grid-stride), block = 256; a lane owns 4 consecutive sites.
// out[s] = {first slot, tag}.  bad: min over illegal characters of t * L + s.
__global__ __launch_bounds__(MSA_WG) void k_msa_hash(const uint8_t * __restrict__ in, size_t Lp, unsigned T, unsigned L,
                                                      MsaCodes codes, unsigned long long keep, unsigned slot_mask,
                                                      uint2 * __restrict__ out, unsigned long long * bad)
{
  __shared__ uint16_t lds[256];
  msa_load_codes(lds, codes);
  const size_t ngroups = ((size_t)L + 3u) / 4u;
  unsigned long long worst = MSA_NO_BAD;
  for (size_t g = (size_t)blockIdx.x * MSA_WG + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * MSA_WG)
  {
    const size_t s0 = 4u * g;
    unsigned long long h1a = 0xcbf29ce484222325ULL, h1b = h1a, h1c = h1a, h1d = h1a;
    unsigned long long h2a = 0x84222325cbf29ce4ULL, h2b = h2a, h2c = h2a, h2d = h2a;
    const uint32_t * col = reinterpret_cast<const uint32_t *>(in + s0);
    const size_t stride = Lp / 4u;
#define MSA_STEP(h1, h2, k, t_)                                                                                   \
    {                                                                                                             \
      const unsigned c = lds[(w >> (8 * (k))) & 255u];                                                            \
      if (c == MSA_ILLEGAL && s0 + (k) < L)                                                                       \
      {                                                                                                           \
        const unsigned long long at = (unsigned long long)(t_) * L + s0 + (k);                                    \
        worst = at < worst ? at : worst;                                                                          \
      }                                                                                                           \
      h1 = (h1 ^ c) * 0x100000001b3ULL;                                                                           \
      h2 = (h2 + c + 1u) * 0x9e3779b97f4a7c15ULL;                                                                 \
    }
#define MSA_WORD(w_, t_)                                                                                          \
    {                                                                                                             \
      const uint32_t w = (w_);                                                                                    \
      MSA_STEP(h1a, h2a, 0, t_) MSA_STEP(h1b, h2b, 1, t_) MSA_STEP(h1c, h2c, 2, t_) MSA_STEP(h1d, h2d, 3, t_)     \
    }
    unsigned t = 0;
    for (; t + 4u <= T; t += 4u)
    {
      const uint32_t w0 = col[(size_t)t * stride], w1 = col[(size_t)(t + 1u) * stride];
      const uint32_t w2 = col[(size_t)(t + 2u) * stride], w3 = col[(size_t)(t + 3u) * stride];
      MSA_WORD(w0, t) MSA_WORD(w1, t + 1u) MSA_WORD(w2, t + 2u) MSA_WORD(w3, t + 3u)
    }
    for (; t < T; ++t) MSA_WORD(col[(size_t)t * stride], t)
#undef MSA_WORD
#undef MSA_STEP
#define MSA_OUT(h1, h2, k)                                                                                        \
    if (s0 + (k) < L)                                                                                             \
      out[s0 + (k)] = make_uint2((unsigned)(msa_fmix(h1, 0xff51afd7ed558ccdULL, 0xc4ceb9fe1a85ec53ULL) & keep) & slot_mask, \
                                 (unsigned)(msa_fmix(h2, 0xbf58476d1ce4e5b9ULL, 0x94d049bb133111ebULL) & keep));
    MSA_OUT(h1a, h2a, 0) MSA_OUT(h1b, h2b, 1) MSA_OUT(h1c, h2c, 2) MSA_OUT(h1d, h2d, 3)
#undef MSA_OUT
  }
  if (worst != MSA_NO_BAD) atomicMin(bad, worst);
}

// columns a and b hold the same canonical codes
__device__ inline bool msa_columns_equal(const uint8_t * in, size_t Lp, unsigned T, const uint16_t * lds, unsigned a,
                                         unsigned b)
{
  const uint8_t * pa = in + a, * pb = in + b;
  unsigned t = 0;
  for (; t + 4u <= T; t += 4u, pa += 4u * Lp, pb += 4u * Lp)
  {
    const unsigned a0 = pa[0], a1 = pa[Lp], a2 = pa[2u * Lp], a3 = pa[3u * Lp];
    const unsigned b0 = pb[0], b1 = pb[Lp], b2 = pb[2u * Lp], b3 = pb[3u * Lp];
    if ((lds[a0] != lds[b0]) | (lds[a1] != lds[b1]) | (lds[a2] != lds[b2]) | (lds[a3] != lds[b3])) return false;
  }
  for (; t < T; ++t, pa += Lp, pb += Lp)
    if (lds[*pa] != lds[*pb]) return false;
  return true;
}

// groups of equal columns.  grid = chunks of 256 sites (grid-stride), block = 256, a site per lane.
// table: slot_mask + 1 slots, all MSA_EMPTY.  owner[s] = the site that owns the slot of s's group;
// first[owner] = min site of the group (all 0xffffffff before), weight[owner] = its size (all 0 before).
// counts[0] += slots passed over (probe steps beyond a site's first slot), counts[1] += full column compares.
__global__ __launch_bounds__(MSA_WG) void k_msa_insert(const uint8_t * __restrict__ in, size_t Lp, unsigned T, unsigned L,
                                                        MsaCodes codes, const uint2 * __restrict__ hash,
                                                        unsigned long long * table, unsigned slot_mask,
                                                        unsigned * __restrict__ owner, unsigned * first, unsigned * weight,
                                                        unsigned long long * counts)
{
  __shared__ uint16_t lds[256];
  msa_load_codes(lds, codes);
  const unsigned lane = threadIdx.x & 63u;
  for (size_t base = (size_t)blockIdx.x * MSA_WG + (threadIdx.x & ~63u); base < L; base += (size_t)gridDim.x * MSA_WG)
  {
    const size_t site = base + lane;
    const bool valid = site < L;
    const unsigned s = (unsigned)site;
    unsigned own = 0xffffffffu, nprobe = 0, ncompare = 0;
    if (valid)
    {
      const uint2 h = hash[s];
      const unsigned long long entry = ((unsigned long long)h.y << 32) | s;
      for (unsigned i = h.x; ; i = (i + 1u) & slot_mask, ++nprobe)
      {
        unsigned long long old = __hip_atomic_load(table + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == MSA_EMPTY)
        {
          old = atomicCAS(table + i, MSA_EMPTY, entry);
          if (old == MSA_EMPTY) { own = s; break; }
        }
        if ((unsigned)(old >> 32) == h.y)
        {
          ++ncompare;
          if (msa_columns_equal(in, Lp, T, lds, s, (unsigned)old))
          {
            own = (unsigned)old;
            break;
          }
        }
      }
      owner[s] = own;
    }
    // one pair of atomics per (wave, group): an alignment of identical columns is L updates of one address otherwise.
    // The lowest lane of a group holds its lowest site of this wave.
    unsigned long long todo = __ballot(valid);
    while (todo)
    {
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned lead_own = __shfl(own, leader, 64);
      const unsigned long long same = __ballot(valid && own == lead_own);
      if ((int)lane == leader)
      {
        atomicAdd(weight + own, (unsigned)__popcll(same));
        atomicMin(first + own, s);
      }
      todo &= ~same;
    }
    for (int off = 32; off; off >>= 1)
    {
      nprobe += __shfl_down(nprobe, off, 64);
      ncompare += __shfl_down(ncompare, off, 64);
    }
    if (lane == 0u && (nprobe | ncompare))
    {
      atomicAdd(counts, (unsigned long long)nprobe);
      atomicAdd(counts + 1, (unsigned long long)ncompare);
    }
  }
}

// "site s is the first of its group"
__device__ inline unsigned msa_is_first(const unsigned * owner, const unsigned * first, size_t s)
{
  return first[owner[s]] == (unsigned)s ? 1u : 0u;
}

// Exclusive prefix sum in three launches: sums of 4096-entry tiles, the prefix of those (one workgroup when there
// are at most 1024 of them, else this scheme again on the tile sums), then the entries.
// MARK: the entries are msa_is_first(s); else they are src[].  grid = tiles, block = 1024
template <bool MARK>
__global__ __launch_bounds__(1024) void k_msa_scan_tiles(const unsigned * src, const unsigned * owner,
                                                          const unsigned * first, unsigned n, unsigned * tile_sum)
{
  __shared__ unsigned part[16];
  unsigned v = 0;
  const size_t base = (size_t)blockIdx.x * MSA_SCAN_TILE + threadIdx.x * 4u;
  for (unsigned u = 0; u < 4; ++u)
    if (base + u < n) v += MARK ? msa_is_first(owner, first, base + u) : src[base + u];
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) { unsigned t = 0; for (int w = 0; w < 16; ++w) t += part[w]; tile_sum[blockIdx.x] = t; }
}

// ntiles <= 1024: tile_sum becomes its exclusive prefix, *total the sum.  grid = 1, block = 1024
__global__ __launch_bounds__(1024) void k_msa_scan_top(unsigned * tile_sum, unsigned ntiles, unsigned * total)
{
  __shared__ unsigned buf[1024];
  const unsigned v = threadIdx.x < ntiles ? tile_sum[threadIdx.x] : 0u;
  buf[threadIdx.x] = v;
  __syncthreads();
  for (unsigned off = 1; off < 1024; off <<= 1)
  {
    const unsigned add = threadIdx.x >= off ? buf[threadIdx.x - off] : 0u;
    __syncthreads();
    buf[threadIdx.x] += add;
    __syncthreads();
  }
  if (threadIdx.x < ntiles) tile_sum[threadIdx.x] = buf[threadIdx.x] - v;
  if (threadIdx.x == 1023) *total = buf[1023];
}

// MARK: the first site s of pattern p gets rank[s] = p, pat_site[p] = s, pat_weight[p] = the group's size;
// else src[] becomes its exclusive prefix in place.  tile_sum: exclusive prefix of the tiles.  grid = tiles, block = 1024
template <bool MARK>
__global__ __launch_bounds__(1024) void k_msa_scan_apply(unsigned * src, const unsigned * owner, const unsigned * first,
                                                          const unsigned * weight, unsigned n, const unsigned * tile_sum,
                                                          unsigned * rank, unsigned * pat_site, unsigned * pat_weight)
{
  __shared__ unsigned part[16];
  const size_t base = (size_t)blockIdx.x * MSA_SCAN_TILE + threadIdx.x * 4u;
  unsigned f0 = 0, f1 = 0, f2 = 0, f3 = 0;
  if (base < n) f0 = MARK ? msa_is_first(owner, first, base) : src[base];
  if (base + 1u < n) f1 = MARK ? msa_is_first(owner, first, base + 1u) : src[base + 1u];
  if (base + 2u < n) f2 = MARK ? msa_is_first(owner, first, base + 2u) : src[base + 2u];
  if (base + 3u < n) f3 = MARK ? msa_is_first(owner, first, base + 3u) : src[base + 3u];
  const unsigned v = f0 + f1 + f2 + f3;
  unsigned incl = v;
  for (int off = 1; off < 64; off <<= 1)
  {
    const unsigned t = __shfl_up(incl, off, 64);
    if ((threadIdx.x & 63) >= (unsigned)off) incl += t;
  }
  if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = incl;
  __syncthreads();
  unsigned before = tile_sum[blockIdx.x];
  for (unsigned w = 0; w < (threadIdx.x >> 6); ++w) before += part[w];
  unsigned id = before + incl - v;
#define MSA_APPLY(f, u)                                                                                           \
  if (base + (u) < n)                                                                                             \
  {                                                                                                               \
    if (!MARK) src[base + (u)] = id;                                                                              \
    else if (f)                                                                                                   \
    {                                                                                                             \
      rank[base + (u)] = id;                                                                                      \
      pat_site[id] = (unsigned)(base + (u));                                                                      \
      pat_weight[id] = weight[owner[base + (u)]];                                                                 \
    }                                                                                                             \
    id += f;                                                                                                      \
  }
  MSA_APPLY(f0, 0u) MSA_APPLY(f1, 1u) MSA_APPLY(f2, 2u) MSA_APPLY(f3, 3u)
#undef MSA_APPLY
}

// pattern index of every site.  grid = chunks (grid-stride), block = 256
__global__ __launch_bounds__(MSA_WG) void k_msa_number(const unsigned * __restrict__ owner, const unsigned * __restrict__ first,
                                                        const unsigned * __restrict__ rank, unsigned L,
                                                        unsigned * __restrict__ site_pattern)
{
  for (size_t s = (size_t)blockIdx.x * MSA_WG + threadIdx.x; s < L; s += (size_t)gridDim.x * MSA_WG)
    site_pattern[s] = rank[first[owner[s]]];
}

// the characters of the first occurrences.  out: [taxon][Pp], Pp a multiple of 4; a lane gathers 4 consecutive
// patterns of one taxon and stores one word.  grid = (chunks of 1024 patterns (grid-stride), taxa (grid-stride)),
// block = 256
__global__ __launch_bounds__(MSA_WG) void k_msa_gather(const uint8_t * __restrict__ in, size_t Lp, unsigned T, unsigned P,
                                                        size_t Pp, const unsigned * __restrict__ pat_site,
                                                        uint8_t * __restrict__ out)
{
  const size_t ngroups = ((size_t)P + 3u) / 4u;
  for (size_t g = (size_t)blockIdx.x * MSA_WG + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * MSA_WG)
  {
    const size_t p0 = 4u * g;
    const unsigned s0 = pat_site[p0];
    const unsigned s1 = p0 + 1u < P ? pat_site[p0 + 1u] : s0;
    const unsigned s2 = p0 + 2u < P ? pat_site[p0 + 2u] : s0;
    const unsigned s3 = p0 + 3u < P ? pat_site[p0 + 3u] : s0;
    for (unsigned t = blockIdx.y; t < T; t += gridDim.y)
    {
      const uint8_t * row = in + (size_t)t * Lp;
      const uint32_t w = (uint32_t)row[s0] | ((uint32_t)row[s1] << 8) | ((uint32_t)row[s2] << 16) | ((uint32_t)row[s3] << 24);
      *reinterpret_cast<uint32_t *>(out + (size_t)t * Pp + p0) = w;
    }
  }
}

} // namespace pllhip
