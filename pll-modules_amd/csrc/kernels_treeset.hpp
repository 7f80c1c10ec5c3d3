// kernels_treeset.hpp -- splits, distinct splits, RF distances, Felsenstein and transfer support of a tree set
// (pll_treeset_dev.hip; plans and programs: treeset_plan.h; design: DESIGN.md section 16).
//
//   k_ts_splits   a wave builds one normalised split from its interval of the tree's tip order, in LDS, and its hash
//   k_ts_insert   open-addressing table {tag | where the vector is}; a tag match is confirmed by comparing the two
//                 bit vectors in full, so unequal splits never merge whatever the hash does (the scheme of
//                 kernels_compress.hpp).  During a batch a new split's entry points into the batch buffer.
//   k_ts_commit   every new distinct split gets an id and its vector moves to the resident store
//   k_ts_resolve  the ids of every tree, and per id the number of trees that hold it
//   k_ts_sort     a tree's ids ascending (bitonic, one workgroup per tree)
//   k_ts_lookup   ids of the reference tree's splits (TS_NONE: in no tree)
//   k_ts_rf_*     common splits of two id lists: a wave per pair, a binary search per id
//   k_ts_tbe      transfer distances: a lane per reference split, a workgroup walks transfer programs
//   k_cs_*        consensus: candidates ranked by (trees that hold them, content), then a greedy selection in blocks
//                 (described where the kernels are, at the end of this file)
//
// Which split of a group of equal ones owns a slot, and which id it gets, is a race.  Nothing that leaves the device
// depends on either: splits leave as bit vectors and are ordered by content, RF and FBP count equal ids, and TBE does
// not use ids at all.  Integer work throughout; no floating point.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "treeset_plan.h"

namespace pllhip {

constexpr unsigned TS_WG = 256;
constexpr unsigned TS_NONE = 0xffffffffu;
constexpr unsigned TS_BATCH_FLAG = 0x80000000u;                // entry / owner: an index into the batch buffer
constexpr unsigned long long TS_EMPTY = ~0ULL;
constexpr unsigned TS_NOP = 2u;                                // program padding (treeset_plan.h has PUSH and COMBINE)
constexpr unsigned TS_CHUNK = 4u;                              // steps per load of the transfer kernel

__device__ inline unsigned long long ts_wave_sum(unsigned long long v)
{
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

// grid-stride over rounds of 4 splits, block = 256, dynamic LDS = 4 * len words.
// order [ntrees][T - 1], lohi [ntrees][R] (lo | hi << 16); vec [ntrees * R][len], hash [ntrees * R]
__global__ __launch_bounds__(TS_WG) void k_ts_splits(const uint16_t * __restrict__ order, const uint32_t * __restrict__ lohi,
                                                     unsigned T, unsigned len, unsigned R, size_t nsplits,
                                                     unsigned long long all_keys, uint32_t * __restrict__ vec,
                                                     unsigned long long * __restrict__ hash)
{
  extern __shared__ uint32_t ts_lds[];
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  uint32_t * bits = ts_lds + (size_t)wave * len;
  const uint32_t last = (T & 31u) ? ((1u << (T & 31u)) - 1u) : 0xffffffffu;
  for (size_t base = (size_t)blockIdx.x * 4u; base < nsplits; base += (size_t)gridDim.x * 4u)
  {
    const size_t q = base + wave;
    const bool live = q < nsplits;
    for (unsigned w = lane; w < len; w += 64u) bits[w] = w + 1u == len ? last : 0xffffffffu;
    __syncthreads();
    unsigned long long h = 0;
    if (live)
    {
      const size_t tree = q / R;
      const uint32_t iv = lohi[q];
      const uint16_t * tips = order + tree * (T - 1u);
      for (unsigned k = (iv & 0xffffu) + lane; k < (iv >> 16); k += 64u)
      {
        const unsigned t = tips[k];
        atomicAnd(bits + (t >> 5), ~(1u << (t & 31u)));
        h += pllhip_ts_key(t);
      }
    }
    h = ts_wave_sum(h);
    __syncthreads();
    if (live)
    {
      for (unsigned w = lane; w < len; w += 64u) vec[q * len + w] = bits[w];
      if (lane == 0u) hash[q] = all_keys - h;
    }
    __syncthreads();
  }
}

__device__ inline bool ts_equal(const uint32_t * a, const uint32_t * b, unsigned len)
{
  for (unsigned w = 0; w < len; ++w)
    if (a[w] != b[w]) return false;
  return true;
}

__device__ inline const uint32_t * ts_vector(unsigned where, const uint32_t * store, const uint32_t * batch, unsigned len)
{
  return (where & TS_BATCH_FLAG) ? batch + (size_t)(where & ~TS_BATCH_FLAG) * len : store + (size_t)where * len;
}

// a split per lane.  owner[q]: id of the resident split equal to q, or TS_BATCH_FLAG | the batch split that owns the
// slot (q itself for a new one); slot_of[q]: that slot.  counts[0] += slots passed over, counts[1] += full compares.
__global__ __launch_bounds__(TS_WG) void k_ts_insert(const uint32_t * __restrict__ batch, const unsigned long long * __restrict__ hash,
                                                     const uint32_t * __restrict__ store, unsigned len, unsigned n,
                                                     unsigned long long keep, unsigned long long * table, unsigned slot_mask,
                                                     unsigned * __restrict__ owner, unsigned * __restrict__ slot_of,
                                                     unsigned long long * counts)
{
  for (size_t base = (size_t)blockIdx.x * TS_WG; base < n; base += (size_t)gridDim.x * TS_WG)
  {
    const size_t at = base + threadIdx.x;
    unsigned nprobe = 0, ncompare = 0;
    if (at < n)
    {
      const unsigned q = (unsigned)at;
      const unsigned long long h = hash[q] & keep;
      const unsigned tag = (unsigned)(h >> 32);
      const unsigned long long entry = ((unsigned long long)tag << 32) | TS_BATCH_FLAG | q;
      const uint32_t * mine = batch + (size_t)q * len;
      for (unsigned i = (unsigned)h & slot_mask; ; i = (i + 1u) & slot_mask, ++nprobe)
      {
        unsigned long long old = __hip_atomic_load(table + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == TS_EMPTY)
        {
          old = atomicCAS(table + i, TS_EMPTY, entry);
          if (old == TS_EMPTY) { owner[q] = TS_BATCH_FLAG | q; slot_of[q] = i; break; }
        }
        if ((unsigned)(old >> 32) == tag)
        {
          ++ncompare;
          if (ts_equal(mine, ts_vector((unsigned)old, store, batch, len), len))
          {
            owner[q] = (unsigned)old;
            slot_of[q] = i;
            break;
          }
        }
      }
    }
    for (int off = 32; off; off >>= 1)
    {
      nprobe += __shfl_down(nprobe, off, 64);
      ncompare += __shfl_down(ncompare, off, 64);
    }
    if ((threadIdx.x & 63u) == 0u && (nprobe | ncompare))
    {
      atomicAdd(counts, (unsigned long long)nprobe);
      atomicAdd(counts + 1, (unsigned long long)ncompare);
    }
  }
}

// new distinct splits: id from *ndistinct, vector to the store, the slot now names the id.  The store holds room for
// every split of the batch.
__global__ __launch_bounds__(TS_WG) void k_ts_commit(const uint32_t * __restrict__ batch, const unsigned long long * __restrict__ hash,
                                                     unsigned len, unsigned n, unsigned long long keep,
                                                     const unsigned * __restrict__ owner, const unsigned * __restrict__ slot_of,
                                                     unsigned long long * table, uint32_t * __restrict__ store,
                                                     unsigned * ndistinct, unsigned * __restrict__ new_id)
{
  for (size_t at = (size_t)blockIdx.x * TS_WG + threadIdx.x; at < n; at += (size_t)gridDim.x * TS_WG)
  {
    const unsigned q = (unsigned)at;
    if (owner[q] != (TS_BATCH_FLAG | q)) continue;
    const unsigned id = atomicAdd(ndistinct, 1u);
    new_id[q] = id;
    for (unsigned w = 0; w < len; ++w) store[(size_t)id * len + w] = batch[(size_t)q * len + w];
    table[slot_of[q]] = ((hash[q] & keep) & 0xffffffff00000000ULL) | id;
  }
}

// ids [ntrees][stride] (the tail of every row is TS_NONE already); trees_with[id] += 1
__global__ __launch_bounds__(TS_WG) void k_ts_resolve(const unsigned * __restrict__ owner, const unsigned * __restrict__ new_id,
                                                      unsigned n, unsigned R, unsigned stride, unsigned * __restrict__ ids,
                                                      unsigned * trees_with)
{
  for (size_t at = (size_t)blockIdx.x * TS_WG + threadIdx.x; at < n; at += (size_t)gridDim.x * TS_WG)
  {
    const unsigned o = owner[at];
    const unsigned id = (o & TS_BATCH_FLAG) ? new_id[o & ~TS_BATCH_FLAG] : o;
    ids[(at / R) * stride + at % R] = id;
    atomicAdd(trees_with + id, 1u);
  }
}

// rows of `stride` (a power of two) ids ascending.  grid = trees, block = 256
__global__ __launch_bounds__(TS_WG) void k_ts_sort(unsigned * ids, unsigned stride)
{
  unsigned * v = ids + (size_t)blockIdx.x * stride;
  for (unsigned k = 2; k <= stride; k <<= 1)
    for (unsigned j = k >> 1; j; j >>= 1)
    {
      for (unsigned i = threadIdx.x; i < stride; i += TS_WG)
      {
        const unsigned l = i ^ j;
        if (l > i)
        {
          const unsigned a = v[i], b = v[l];
          if (((i & k) == 0u) == (a > b)) { v[i] = b; v[l] = a; }
        }
      }
      __syncthreads();
    }
}

// id of every reference split.  vec [R][len], hash [R]; a split per lane
__global__ __launch_bounds__(TS_WG) void k_ts_lookup(const uint32_t * __restrict__ vec, const unsigned long long * __restrict__ hash,
                                                     const uint32_t * __restrict__ store, unsigned len, unsigned R,
                                                     unsigned long long keep, const unsigned long long * __restrict__ table,
                                                     unsigned slot_mask, unsigned * __restrict__ ref_id)
{
  for (size_t at = (size_t)blockIdx.x * TS_WG + threadIdx.x; at < R; at += (size_t)gridDim.x * TS_WG)
  {
    const unsigned long long h = hash[at] & keep;
    const unsigned tag = (unsigned)(h >> 32);
    unsigned id = TS_NONE;
    for (unsigned i = (unsigned)h & slot_mask; ; i = (i + 1u) & slot_mask)
    {
      const unsigned long long old = table[i];
      if (old == TS_EMPTY) break;
      if ((unsigned)(old >> 32) == tag && ts_equal(vec + at * len, store + (size_t)(unsigned)old * len, len))
      {
        id = (unsigned)old;
        break;
      }
    }
    ref_id[at] = id;
  }
}

// ids of a[0 .. n) that occur in the ascending list b[0 .. n); the whole wave gets the count
__device__ inline unsigned ts_common(const unsigned * __restrict__ a, const unsigned * __restrict__ b, unsigned n, unsigned lane)
{
  unsigned found = 0;
  for (unsigned k = lane; k < n; k += 64u)
  {
    const unsigned x = a[k];
    if (x == TS_NONE) continue;
    unsigned lo = 0, hi = n;
    while (lo < hi)
    {
      const unsigned mid = (lo + hi) >> 1;
      if (b[mid] < x) lo = mid + 1u; else hi = mid;
    }
    found += (lo < n && b[lo] == x) ? 1u : 0u;
  }
  for (int off = 32; off; off >>= 1) found += __shfl_down(found, off, 64);
  return __shfl(found, 0, 64);
}

// out[j] = 2 * (R - common(reference, tree j)).  a wave per tree
__global__ __launch_bounds__(TS_WG) void k_ts_rf_to(const unsigned * __restrict__ ref_id, const unsigned * __restrict__ ids,
                                                    unsigned stride, unsigned R, unsigned B, unsigned * __restrict__ out)
{
  const unsigned lane = threadIdx.x & 63u;
  for (size_t j = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6); j < B; j += (size_t)gridDim.x * 4u)
  {
    const unsigned c = ts_common(ref_id, ids + j * stride, R, lane);
    if (lane == 0u) out[j] = 2u * (R - c);
  }
}

// out [B][B], zero before: a wave per pair i < j.  grid = (ceil(B / 4), B): blockIdx.y = i, a wave per j
__global__ __launch_bounds__(TS_WG) void k_ts_rf_matrix(const unsigned * __restrict__ ids, unsigned stride, unsigned R, unsigned B,
                                                        unsigned * __restrict__ out)
{
  const unsigned lane = threadIdx.x & 63u;
  for (size_t i = blockIdx.y; i < B; i += gridDim.y)
    for (size_t j = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6); j < B; j += (size_t)gridDim.x * 4u)
    {
      if (j <= i) continue;
      const unsigned c = ts_common(ids + i * stride, ids + j * stride, R, lane);
      if (lane == 0u) out[i * B + j] = out[j * B + i] = 2u * (R - c);
    }
}

// sums[i] = number of trees that hold reference split i
__global__ __launch_bounds__(TS_WG) void k_ts_fbp(const unsigned * __restrict__ ref_id, const unsigned * __restrict__ trees_with,
                                                  unsigned R, unsigned long long * __restrict__ sums)
{
  for (size_t i = (size_t)blockIdx.x * TS_WG + threadIdx.x; i < R; i += (size_t)gridDim.x * TS_WG)
    sums[i] = ref_id[i] == TS_NONE ? 0ULL : (unsigned long long)trees_with[ref_id[i]];
}

// out [R][len]: the vectors of one tree's ids
__global__ __launch_bounds__(TS_WG) void k_ts_gather(const unsigned * __restrict__ ids, const uint32_t * __restrict__ store,
                                                     unsigned len, unsigned R, uint32_t * __restrict__ out)
{
  const size_t n = (size_t)R * len;
  for (size_t at = (size_t)blockIdx.x * TS_WG + threadIdx.x; at < n; at += (size_t)gridDim.x * TS_WG)
    out[at] = store[(size_t)ids[at / len] * len + at % len];
}

// Transfer distances.  A lane owns reference split i = 64 * group + lane; a wave owns a group; the workgroup's four
// waves walk the same programs.  programs [B][nsteps], nsteps a multiple of TS_CHUNK (padded with TS_NOP); ref_bits
// [T][groups]: bit `lane` of word (t, group) = tip t is in split 64 * group + lane; ones_of[i] = popcount of split i.
// Step and bit loads are wave-uniform (scalar); the four of a chunk are issued before any is used.  The stack of
// 16-bit counts lives in LDS as [entry][lane] with its top entry in a register: a lane touches only its own column,
// so no barrier.  sums[i] += min(p - 1, min over nodes v of min(d, T - d)), d = |split i xor tips below v|.
// grid = (ceil(groups / 4), tree slices), block = 256
__global__ __launch_bounds__(TS_WG) void k_ts_tbe(const uint2 * __restrict__ programs, unsigned nsteps,
                                                  const unsigned long long * __restrict__ ref_bits, unsigned groups,
                                                  const uint16_t * __restrict__ ones_of, unsigned R, unsigned T, unsigned B,
                                                  unsigned long long * sums)
{
  __shared__ uint16_t stack[PLLHIP_TS_MAX_STACK][TS_WG];
  const unsigned lane = threadIdx.x & 63u;
  const unsigned group = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
  if (group >= groups) return;
  const unsigned i = group * 64u + lane;
  const unsigned p = i < R ? ones_of[i] : 2u;
  const unsigned cap = (p < T - p ? p : T - p) - 1u;
  unsigned long long acc = 0;
  for (unsigned tree = blockIdx.y; tree < B; tree += gridDim.y)
  {
    const uint2 * prog = programs + (size_t)tree * nsteps;
    unsigned delta = cap, sp = 0, top = 0;
    for (unsigned s = 0; s < nsteps; s += TS_CHUNK)
    {
      uint2 st[TS_CHUNK];
      unsigned long long word[TS_CHUNK];
#pragma unroll
      for (unsigned u = 0; u < TS_CHUNK; ++u) st[u] = prog[s + u];
      // a combine's argument is a size below T and a NOP's is 0: every argument names a row
#pragma unroll
      for (unsigned u = 0; u < TS_CHUNK; ++u) word[u] = ref_bits[(size_t)st[u].y * groups + group];
#pragma unroll
      for (unsigned u = 0; u < TS_CHUNK; ++u)
      {
        if (st[u].x == PLLHIP_TS_PUSH)
        {
          if (sp) stack[sp - 1u][threadIdx.x] = (uint16_t)top;
          top = (unsigned)(word[u] >> lane) & 1u;
          ++sp;
        }
        else if (st[u].x == PLLHIP_TS_COMBINE)
        {
          --sp;
          top += stack[sp - 1u][threadIdx.x];
          const unsigned d = p + st[u].y - 2u * top;
          const unsigned e = T - d;
          delta = min(delta, min(d, e));
        }
      }
    }
    acc += delta;
  }
  if (i < R) atomicAdd(sums + i, acc);
}

// ---- consensus --------------------------------------------------------------------------
// Candidates are the distinct splits held by at least need_minor trees.  Their rank is (trees descending, bit vector
// ascending, word 0 first): content, never an id.  A rank entry is {key, id} with key = ~trees << 32 | word 0, so the
// key alone decides all but ties in trees and word 0; those are settled by comparing the two rows of the store.
// Splits held by need_major trees or more are pairwise compatible and are accepted as they stand; the others go
// through the greedy selection in blocks of n <= CS_MAX_BLOCK candidates:
//   k_cs_filter   a wave per candidate: against every accepted split, stopping at the first incompatible one
//   k_cs_pairs    a wave per survivor i: against the survivors j < i of the block; conflict[i] is a row of bits
//   k_cs_resolve  one workgroup: wave 0 walks the block in rank order and takes survivor i when conflict[i] has no bit
//                 in common with the survivors taken so far; then all four waves append the taken vectors
// Two normalised splits (both hold tip 0) are compatible exactly when one holds the other or their union is every tip.
// A wave tests 64 / G splits at a time, G = the power of two >= len (at most 64) lanes per split, lanes striding over
// words; three ballots carry the three properties and a fold per group decides.
// state: {held, candidates, majority, unused}; tests: {candidate-accepted tests, pairwise tests}.

constexpr unsigned CS_MAX_BLOCK = 2048;                        // 64 lanes x 32 bits: a conflict row fits a wave
constexpr unsigned CS_HELD = 0, CS_NCAND = 1, CS_NMAJOR = 2;

struct CsEntry { unsigned long long key; unsigned id; unsigned pad; };

__global__ __launch_bounds__(TS_WG) void k_cs_candidates(const unsigned * __restrict__ trees_with, const uint32_t * __restrict__ store,
                                                         unsigned len, unsigned D, unsigned need_major, unsigned need_minor,
                                                         CsEntry * __restrict__ rank, unsigned * state)
{
  for (size_t at = (size_t)blockIdx.x * TS_WG + threadIdx.x; at < D; at += (size_t)gridDim.x * TS_WG)
  {
    const unsigned c = trees_with[at];
    if (c < need_minor) continue;
    const unsigned slot = atomicAdd(state + CS_NCAND, 1u);
    if (c >= need_major) atomicAdd(state + CS_NMAJOR, 1u);
    CsEntry e;
    e.key = ((unsigned long long)(~c) << 32) | store[at * len];
    e.id = (unsigned)at;
    e.pad = 0u;
    rank[slot] = e;
  }
}

// rank[from .. n) = padding that sorts last
__global__ __launch_bounds__(TS_WG) void k_cs_pad(CsEntry * __restrict__ rank, const unsigned * __restrict__ state, unsigned n)
{
  const unsigned from = state[CS_NCAND];
  for (size_t at = (size_t)blockIdx.x * TS_WG + threadIdx.x + from; at < n; at += (size_t)gridDim.x * TS_WG)
  {
    CsEntry e;
    e.key = ~0ULL; e.id = TS_NONE; e.pad = 0u;
    rank[at] = e;
  }
}

__device__ inline bool cs_after(const CsEntry & a, const CsEntry & b, const uint32_t * __restrict__ store, unsigned len)
{
  if (a.key != b.key) return a.key > b.key;
  if (a.id == b.id || a.id == TS_NONE || b.id == TS_NONE) return false;
  const uint32_t * x = store + (size_t)a.id * len, * y = store + (size_t)b.id * len;
  for (unsigned w = 1; w < len; ++w)
    if (x[w] != y[w]) return x[w] > y[w];
  return false;
}

// one step (k, j) of a bitonic sort of n = 2^m entries in global memory
__global__ __launch_bounds__(TS_WG) void k_cs_sort_step(CsEntry * rank, unsigned n, unsigned k, unsigned j,
                                                        const uint32_t * __restrict__ store, unsigned len)
{
  for (size_t at = (size_t)blockIdx.x * TS_WG + threadIdx.x; at < n; at += (size_t)gridDim.x * TS_WG)
  {
    const unsigned i = (unsigned)at, l = i ^ j;
    if (l <= i) continue;
    const CsEntry a = rank[i], b = rank[l];
    if (((i & k) == 0u) ? cs_after(a, b, store, len) : cs_after(b, a, store, len)) { rank[i] = b; rank[l] = a; }
  }
}

// all the steps j <= TS_WG of one k, or (k == 0) the whole sort of every 2 * TS_WG entries, in LDS
__global__ __launch_bounds__(TS_WG) void k_cs_sort_local(CsEntry * rank, unsigned n, unsigned k_from, unsigned k_to,
                                                         const uint32_t * __restrict__ store, unsigned len)
{
  __shared__ CsEntry tile[2u * TS_WG];
  for (size_t base = (size_t)blockIdx.x * 2u * TS_WG; base < n; base += (size_t)gridDim.x * 2u * TS_WG)
  {
    for (unsigned i = threadIdx.x; i < 2u * TS_WG; i += TS_WG)
    {
      if (base + i < n) tile[i] = rank[base + i];
      else { tile[i].key = ~0ULL; tile[i].id = TS_NONE; tile[i].pad = 0u; }
    }
    __syncthreads();
    for (unsigned k = k_from; k <= k_to; k <<= 1)
      for (unsigned j = min(k >> 1, TS_WG); j; j >>= 1)
      {
        const unsigned i = 2u * threadIdx.x - (threadIdx.x & (j - 1u)), l = i + j;      // the pair's lower index
        const bool up = (((unsigned)base + i) & k) == 0u;
        const CsEntry a = tile[i], b = tile[l];
        if (up ? cs_after(a, b, store, len) : cs_after(b, a, store, len)) { tile[i] = b; tile[l] = a; }
        __syncthreads();
      }
    for (unsigned i = threadIdx.x; i < 2u * TS_WG; i += TS_WG)
      if (base + i < n) rank[base + i] = tile[i];
    __syncthreads();
  }
}

// accepted[i] = the vector of rank[i], i < min(majority, R); held = that many
__global__ __launch_bounds__(TS_WG) void k_cs_take_majority(const CsEntry * __restrict__ rank, const uint32_t * __restrict__ store,
                                                            const unsigned * __restrict__ trees_with, unsigned len, unsigned R,
                                                            uint32_t * __restrict__ accepted, unsigned * __restrict__ acc_trees,
                                                            unsigned * state)
{
  const unsigned m = min(state[CS_NMAJOR], R);
  const size_t n = (size_t)m * len;
  for (size_t at = (size_t)blockIdx.x * TS_WG + threadIdx.x; at < n; at += (size_t)gridDim.x * TS_WG)
  {
    const unsigned id = rank[at / len].id;
    accepted[at] = store[(size_t)id * len + at % len];
    if (at % len == 0u) acc_trees[at / len] = trees_with[id];
  }
  if (blockIdx.x == 0u && threadIdx.x == 0u) state[CS_HELD] = m;     // read by later kernels only
}

// the groups (of G lanes, bit g * G) whose split is incompatible with the wave's own: every property has a lane
__device__ inline unsigned long long cs_bad_groups(bool a_outside_b, bool b_outside_a, bool missing, unsigned G)
{
  unsigned long long x = __ballot(a_outside_b), y = __ballot(b_outside_a), z = __ballot(missing);
  for (unsigned s = 1; s < G; s <<= 1) { x |= x >> s; y |= y >> s; z |= z >> s; }
  return x & y & z;
}

__device__ inline unsigned long long cs_group_heads(unsigned G)
{
  unsigned long long m = 0;
  for (unsigned b = 0; b < 64u; b += G) m |= 1ULL << b;
  return m;
}

// `mine` against rows[0 .. count), 64 / G of them at a time: true when compatible with all; it stops after the first
// group that holds an incompatible row.  tests += rows looked at.
__device__ inline bool cs_against(const uint32_t * __restrict__ mine, const uint32_t * __restrict__ rows, unsigned count,
                                  unsigned len, uint32_t last, unsigned G, unsigned lane, unsigned long long & tests)
{
  const unsigned per = 64u / G, sub = lane / G, w0 = lane % G;
  const unsigned long long heads = cs_group_heads(G);
  for (unsigned base = 0; base < count; base += per)
  {
    const unsigned s = base + sub;
    bool f1 = false, f2 = false, f3 = false;
    if (s < count)
      for (unsigned w = w0; w < len; w += G)
      {
        const uint32_t a = mine[w], b = rows[(size_t)s * len + w];
        f1 |= (a & ~b) != 0u;
        f2 |= (b & ~a) != 0u;
        f3 |= (~(a | b) & (w + 1u == len ? last : 0xffffffffu)) != 0u;
      }
    tests += min(per, count - base);
    if (cs_bad_groups(f1, f2, f3, G) & heads) return false;
  }
  return true;
}

// a wave per candidate rank[first + i], i < n: survives[i] = compatible with accepted[0 .. held)
__global__ __launch_bounds__(TS_WG) void k_cs_filter(const CsEntry * __restrict__ rank, unsigned first, unsigned n,
                                                     const uint32_t * __restrict__ store, const uint32_t * __restrict__ accepted,
                                                     unsigned len, unsigned T, unsigned R, unsigned G,
                                                     const unsigned * __restrict__ state, unsigned * __restrict__ survives,
                                                     unsigned long long * tests)
{
  const unsigned held = state[CS_HELD], lane = threadIdx.x & 63u;
  if (held >= R) return;
  const uint32_t last = (T & 31u) ? ((1u << (T & 31u)) - 1u) : 0xffffffffu;
  unsigned long long done = 0;
  for (unsigned i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u)
  {
    const uint32_t * mine = store + (size_t)rank[first + i].id * len;
    const bool ok = cs_against(mine, accepted, held, len, last, G, lane, done);
    if (lane == 0u) survives[i] = ok ? 1u : 0u;
  }
  if (lane == 0u && done) atomicAdd(tests, done);
}

// a wave per candidate i of the block: conflict[i][w], bit j % 32 of word j / 32 = survivors i and j < i are
// incompatible.  rowwords = ceil(n / 32) <= 64
__global__ __launch_bounds__(TS_WG) void k_cs_pairs(const CsEntry * __restrict__ rank, unsigned first, unsigned n,
                                                    const uint32_t * __restrict__ store, unsigned len, unsigned T, unsigned R,
                                                    unsigned G, const unsigned * __restrict__ state,
                                                    const unsigned * __restrict__ survives, uint32_t * __restrict__ conflict,
                                                    unsigned rowwords, unsigned long long * tests)
{
  const unsigned lane = threadIdx.x & 63u;
  if (state[CS_HELD] >= R) return;
  const uint32_t last = (T & 31u) ? ((1u << (T & 31u)) - 1u) : 0xffffffffu;
  const unsigned per = 64u / G, sub = lane / G, w0 = lane % G;
  const unsigned long long heads = cs_group_heads(G);
  unsigned long long done = 0;
  for (unsigned i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u)
  {
    uint32_t row = 0;                                          // lane w holds word w of the row
    if (survives[i])
    {
      const uint32_t * mine = store + (size_t)rank[first + i].id * len;
      for (unsigned base = 0; base < i; base += per)
      {
        const unsigned j = base + sub;
        const bool live = j < i && survives[j] != 0u;
        bool f1 = false, f2 = false, f3 = false;
        if (live)
        {
          const uint32_t * other = store + (size_t)rank[first + j].id * len;
          for (unsigned w = w0; w < len; w += G)
          {
            const uint32_t a = mine[w], b = other[w];
            f1 |= (a & ~b) != 0u;
            f2 |= (b & ~a) != 0u;
            f3 |= (~(a | b) & (w + 1u == len ? last : 0xffffffffu)) != 0u;
          }
        }
        done += (unsigned long long)__popcll(__ballot(live) & heads);
        unsigned long long bad = cs_bad_groups(f1, f2, f3, G) & heads;
        for (; bad; bad &= bad - 1ULL)
        {
          const unsigned j_bad = base + ((unsigned)__ffsll((long long)bad) - 1u) / G;
          if (lane == j_bad / 32u) row |= 1u << (j_bad % 32u);
        }
      }
    }
    if (lane < rowwords) conflict[(size_t)i * rowwords + lane] = row;
  }
  if (lane == 0u && done) atomicAdd(tests, done);
}

// one workgroup.  Wave 0 walks the block in rank order; then every thread appends the taken vectors.
__global__ __launch_bounds__(TS_WG) void k_cs_resolve(const CsEntry * __restrict__ rank, unsigned first, unsigned n,
                                                      const uint32_t * __restrict__ store, const unsigned * __restrict__ trees_with,
                                                      unsigned len, unsigned R, const unsigned * __restrict__ survives,
                                                      const uint32_t * __restrict__ conflict, unsigned rowwords,
                                                      uint32_t * __restrict__ accepted, unsigned * __restrict__ acc_trees,
                                                      unsigned * state)
{
  __shared__ unsigned short taken_at[CS_MAX_BLOCK];            // the block index of the k-th split taken
  __shared__ unsigned ntaken;
  const unsigned held = state[CS_HELD];
  if (held >= R) return;
  if (threadIdx.x < 64u)
  {
    const unsigned lane = threadIdx.x;
    uint32_t taken = 0;                                        // lane w: word w of the set of survivors taken
    unsigned count = 0;
    for (unsigned base = 0; base < n && held + count < R; base += 64u)
    {
      // the survivors among 64 candidates at once: most rounds have few
      unsigned long long live = __ballot(base + lane < n && survives[base + lane] != 0u);
      for (; live && held + count < R; live &= live - 1ULL)
      {
        const unsigned i = base + (unsigned)__ffsll((long long)live) - 1u;
        const uint32_t row = lane < rowwords ? conflict[(size_t)i * rowwords + lane] : 0u;
        if (__ballot((row & taken) != 0u)) continue;
        if (lane == i / 32u) taken |= 1u << (i % 32u);
        if (lane == 0u) taken_at[count] = (unsigned short)i;
        ++count;
      }
    }
    if (lane == 0u) ntaken = count;
  }
  __syncthreads();
  const unsigned count = ntaken;
  for (unsigned at = threadIdx.x; at < count * len; at += TS_WG)
  {
    const unsigned k = at / len, w = at % len, id = rank[first + taken_at[k]].id;
    accepted[(size_t)(held + k) * len + w] = store[(size_t)id * len + w];
    if (w == 0u) acc_trees[held + k] = trees_with[id];
  }
  __syncthreads();
  if (threadIdx.x == 0u) state[CS_HELD] = held + count;
}

} // namespace pllhip
