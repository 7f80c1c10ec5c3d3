// pll_treeset_dev.hip -- pllhip_treeset_*: a set of trees on the device and what is computed from it: normalised
// splits, Robinson-Foulds distances, Felsenstein and transfer bootstrap support, and the consensus of the set
// (kernels_treeset.hpp; host side: host/pllhip_treeset.c, host/pllhip_consensus.c; contract: INTEGRATION.md, "Split
// support and tree distances"; design: DESIGN.md sections 16 and 17).
//
// The host keeps every tree's split plan and transfer program (O(T) each); pllhip_treeset_add touches no device.  The
// device holds a cache of them: the programs, the distinct splits' bit vectors, the hash table over those and every
// tree's sorted split ids.  A query first brings the cache up to date, batch by batch, on a stream of its own; a
// query that fails drops the cache, so the set is as it was and the next query builds it again.
#include "device_job.hpp"
#include "kernels_treeset.hpp"
#include "pllhip.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pllhip;

struct pllhip_treeset
{
  unsigned T = 0, len = 0, R = 0, stride = 0, nsteps = 0;     // tips, words per split, splits per tree, id row, steps
  pllhip_ts_labels_t * labels = nullptr;
  unsigned count = 0;
  std::vector<uint16_t> order;                                 // [count][T - 1]
  std::vector<uint32_t> lohi;                                  // [count][R]
  std::vector<uint2> program;                                  // [count][nsteps]
  std::vector<unsigned> max_stack;                             // [count]

  // the device cache
  int device = -1;
  unsigned ingested = 0, capacity = 0;                         // trees on the device; trees it has room for
  uint2 * d_program = nullptr;
  unsigned * d_ids = nullptr;                                  // [capacity][stride], rows ascending, TS_NONE tails
  unsigned long long * d_table = nullptr;
  size_t slots = 0;
  uint32_t * d_store = nullptr;                                // [store_cap][len]
  unsigned * d_trees_with = nullptr;                           // [store_cap]
  size_t store_cap = 0;
  unsigned long long * d_scalars = nullptr;                    // {distinct splits (low word), probe steps, compares}
  unsigned ndistinct = 0;
};

namespace {

thread_local double g_last_ms[3] = {0.0, 0.0, 0.0};
thread_local unsigned long long g_last_counts[2] = {0, 0};
thread_local std::vector<unsigned long long> g_last_sums;
thread_local unsigned long long g_last_consensus[2] = {0, 0};

void drop_cache(pllhip_treeset * ts)
{
  if (ts->device >= 0)
  {
    DeviceScope scope;
    (void)scope.enter(ts->device);
    (void)hipFree(ts->d_program); (void)hipFree(ts->d_ids); (void)hipFree(ts->d_table); (void)hipFree(ts->d_store);
    (void)hipFree(ts->d_trees_with); (void)hipFree(ts->d_scalars);
  }
  ts->d_program = nullptr; ts->d_ids = nullptr; ts->d_table = nullptr; ts->d_store = nullptr;
  ts->d_trees_with = nullptr; ts->d_scalars = nullptr;
  ts->device = -1; ts->ingested = ts->capacity = ts->ndistinct = 0; ts->slots = ts->store_cap = 0;
}

constexpr const char * SPLIT_HASH_BITS = "PLLHIP_SPLIT_HASH_BITS";      // hash_keep_mask: a test knob

unsigned long long all_keys(unsigned T)
{
  unsigned long long all = 0;
  for (unsigned t = 0; t < T; ++t) all += pllhip_ts_key(t);
  return all;
}

// one query: the device, a stream, and the three clocks
struct Job : DeviceJob
{
  hipEvent_t a = nullptr, b = nullptr;
  double ms[3] = {0.0, 0.0, 0.0};

  bool open(pllhip_treeset * ts)
  {
    int device = -1;
    if (!caller_device("the tree set", &device)) return false;
    if (ts->device >= 0 && ts->device != device) drop_cache(ts);
    if (!enter(device) || !(a = event()) || !(b = event())) return false;
    ts->device = device;
    return true;
  }
  // frees a buffer before the query ends
  void release(void * p)
  {
    if (stream) (void)hipStreamSynchronize(stream);
    (void)hipFree(p);
    keep(p);
  }
  bool start() { return hip_ok(hipEventRecord(a, stream), "hipEventRecord"); }
  // ends a segment: the stream is idle afterwards
  bool stop(int which, const char * what)
  {
    float t = 0.f;
    if (!hip_ok(hipGetLastError(), what) || !hip_ok(hipEventRecord(b, stream), "hipEventRecord") ||
        !hip_ok(hipEventSynchronize(b), what) || !elapsed(a, b, &t))
      return false;
    ms[which] += t;
    return true;
  }
  template <typename T> bool temp(T ** ptr, size_t count, const char * what)
  {
    return (*ptr = alloc<T>(count, what)) != nullptr;
  }
  bool up(void * dst, const void * src, size_t bytes)
  {
    return upload(static_cast<char *>(dst), static_cast<const char *>(src), bytes, "upload");
  }
  bool down(void * dst, const void * src, size_t bytes)
  {
    return download(static_cast<char *>(dst), static_cast<const char *>(src), bytes, "download");
  }
  void commit()
  {
    for (int k = 0; k < 3; ++k) g_last_ms[k] = ms[k];
  }
};

// trees per batch: PLLHIP_TREESET_BATCH, else what a quarter of the free memory holds (batch buffer and the store's
// growth are both one vector per split)
unsigned batch_size(const pllhip_treeset * ts, unsigned pending)
{
  const size_t per_tree = (size_t)ts->R * ((size_t)ts->len * 4u * 2u + 32u) + (size_t)ts->T * 2u;
  size_t batch = 0;
  const char * env = getenv("PLLHIP_TREESET_BATCH");
  if (env && *env && atol(env) > 0) batch = (size_t)atol(env);
  else
  {
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) { (void)hipGetLastError(); free_bytes = (size_t)1 << 30; }
    batch = free_bytes / 4u / per_tree;
  }
  batch = std::min(batch, (size_t)0x7ffffff0u / ts->R);        // a batch's splits are numbered in 31 bits
  return (unsigned)std::max<size_t>(1, std::min<size_t>(batch, pending));
}

bool grow_store(pllhip_treeset * ts, Job & j, size_t need)
{
  if (need <= ts->store_cap) return true;
  if (need >= 0x7fffffffu)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "the tree set numbers distinct splits in 31 bits; %zu asked for", need);
    return false;
  }
  const size_t cap = std::min<size_t>(std::max(need, ts->store_cap + ts->store_cap / 2u), 0x7ffffffeu);
  uint32_t * store = nullptr;
  unsigned * with = nullptr;
  if (!dev_alloc(&store, cap * ts->len, "the distinct splits")) return false;
  if (!dev_alloc(&with, cap, "the trees per split")) { (void)hipFree(store); return false; }
  bool ok = hip_ok(hipMemsetAsync(with, 0, cap * sizeof(unsigned), j.stream), "memset");
  if (ok && ts->ndistinct)
    ok = hip_ok(hipMemcpyAsync(store, ts->d_store, (size_t)ts->ndistinct * ts->len * 4u, hipMemcpyDeviceToDevice, j.stream), "copy") &&
         hip_ok(hipMemcpyAsync(with, ts->d_trees_with, (size_t)ts->ndistinct * sizeof(unsigned), hipMemcpyDeviceToDevice, j.stream), "copy");
  ok = ok && hip_ok(hipStreamSynchronize(j.stream), "growing the split store");
  if (!ok) { (void)hipFree(store); (void)hipFree(with); return false; }
  (void)hipFree(ts->d_store); (void)hipFree(ts->d_trees_with);
  ts->d_store = store; ts->d_trees_with = with; ts->store_cap = cap;
  return true;
}

// brings the device cache up to the host's trees
bool sync_cache(pllhip_treeset * ts, Job & j)
{
  if (ts->ingested == ts->count) return true;
  const unsigned B = ts->count, R = ts->R, len = ts->len;
  if (B > ts->capacity)
  {
    // a set that grew after a query: everything again, with room for all of it
    const int device = ts->device;
    drop_cache(ts);
    ts->device = device;
    size_t slots = 2;
    while (slots < 2u * (size_t)B * R) slots <<= 1;
    if (slots > ((size_t)1 << 32)) { set_error(PLL_ERROR_MEM_ALLOC, "the tree set's table would need %zu slots", slots); return false; }
    if (!dev_alloc(&ts->d_program, (size_t)B * ts->nsteps, "transfer programs") ||
        !dev_alloc(&ts->d_ids, (size_t)B * ts->stride, "split ids") || !dev_alloc(&ts->d_table, slots, "the split table") ||
        !dev_alloc(&ts->d_scalars, 3, "scalars"))
      return false;
    ts->slots = slots;
    ts->capacity = B;
    if (!hip_ok(hipMemsetAsync(ts->d_table, 0xff, slots * sizeof(unsigned long long), j.stream), "memset table") ||
        !hip_ok(hipMemsetAsync(ts->d_ids, 0xff, (size_t)B * ts->stride * sizeof(unsigned), j.stream), "memset ids") ||
        !hip_ok(hipMemsetAsync(ts->d_scalars, 0, 3 * sizeof(unsigned long long), j.stream), "memset scalars"))
      return false;
  }
  const unsigned long long keep = hash_keep_mask(SPLIT_HASH_BITS), keys = all_keys(ts->T);
  const unsigned slot_mask = (unsigned)(ts->slots - 1u);
  const unsigned batch = batch_size(ts, B - ts->ingested);
  const size_t nmax = (size_t)batch * R;
  uint16_t * d_order = nullptr;
  uint32_t * d_lohi = nullptr, * d_vec = nullptr;
  unsigned long long * d_hash = nullptr;
  unsigned * d_owner = nullptr, * d_slot = nullptr, * d_new = nullptr;
  if (!j.temp(&d_order, (size_t)batch * (ts->T - 1u), "tip orders") || !j.temp(&d_lohi, nmax, "intervals") ||
      !j.temp(&d_vec, nmax * len, "a batch of splits") || !j.temp(&d_hash, nmax, "split hashes") ||
      !j.temp(&d_owner, nmax, "owners") || !j.temp(&d_slot, nmax, "slots") || !j.temp(&d_new, nmax, "new ids"))
    return false;
  unsigned long long scalars[3];
  while (ts->ingested < B)
  {
    const unsigned first = ts->ingested, nb = std::min(batch, B - first);
    const unsigned n = nb * R;
    if (!grow_store(ts, j, (size_t)ts->ndistinct + n)) return false;
    if (!j.start() || !j.up(d_order, ts->order.data() + (size_t)first * (ts->T - 1u), (size_t)nb * (ts->T - 1u) * 2u) ||
        !j.up(d_lohi, ts->lohi.data() + (size_t)first * R, (size_t)n * 4u) ||
        !j.up(ts->d_program + (size_t)first * ts->nsteps, ts->program.data() + (size_t)first * ts->nsteps,
              (size_t)nb * ts->nsteps * sizeof(uint2)) ||
        !j.stop(0, "uploading trees"))
      return false;
    if (!j.start()) return false;
    hipLaunchKernelGGL(k_ts_splits, dim3(grid_for(n, 4)), dim3(TS_WG), 4u * len * sizeof(uint32_t), j.stream,
                       (const uint16_t *)d_order, (const uint32_t *)d_lohi, ts->T, len, R, (size_t)n, keys, d_vec, d_hash);
    hipLaunchKernelGGL(k_ts_insert, dim3(grid_for(n, TS_WG)), dim3(TS_WG), 0, j.stream, (const uint32_t *)d_vec,
                       (const unsigned long long *)d_hash, (const uint32_t *)ts->d_store, len, n, keep, ts->d_table,
                       slot_mask, d_owner, d_slot, ts->d_scalars + 1);
    hipLaunchKernelGGL(k_ts_commit, dim3(grid_for(n, TS_WG)), dim3(TS_WG), 0, j.stream, (const uint32_t *)d_vec,
                       (const unsigned long long *)d_hash, len, n, keep, (const unsigned *)d_owner, (const unsigned *)d_slot,
                       ts->d_table, ts->d_store, reinterpret_cast<unsigned *>(ts->d_scalars), d_new);
    hipLaunchKernelGGL(k_ts_resolve, dim3(grid_for(n, TS_WG)), dim3(TS_WG), 0, j.stream, (const unsigned *)d_owner,
                       (const unsigned *)d_new, n, R, ts->stride, ts->d_ids + (size_t)first * ts->stride, ts->d_trees_with);
    hipLaunchKernelGGL(k_ts_sort, dim3(nb), dim3(TS_WG), 0, j.stream, ts->d_ids + (size_t)first * ts->stride, ts->stride);
    if (!j.stop(1, "split kernels")) return false;
    if (!j.start() || !j.down(scalars, ts->d_scalars, sizeof(scalars)) || !j.stop(2, "reading the split count")) return false;
    ts->ndistinct = (unsigned)scalars[0];
    if (ts->ndistinct > ts->store_cap)
    {
      set_error(PLL_ERROR_HIP_RUNTIME, "tree set: %u distinct splits counted, room for %zu", ts->ndistinct, ts->store_cap);
      return false;
    }
    ts->ingested = first + nb;
  }
  g_last_counts[0] = scalars[1];
  g_last_counts[1] = scalars[2];
  j.release(d_vec);
  return true;
}

// the reference tree of a query, on the host: splits ascending, their hashes and edges
struct Reference
{
  std::vector<uint32_t> words;                                 // [R][len], ascending
  std::vector<unsigned long long> hash;
  std::vector<pll_unode_t *> edge;
};

bool flatten_reference(const pllhip_treeset * ts, const pll_utree_t * ref, Reference & out)
{
  const unsigned T = ts->T, R = ts->R, len = ts->len;
  std::vector<uint32_t> order(T - 1u), lo(R), hi(R), words((size_t)R * len), perm(R);
  std::vector<pll_unode_t *> edge(R);
  std::vector<pllhip_ts_step_t> program(2u * T - 3u);
  std::vector<uint64_t> hash(R);
  if (!pllhip_ts_flatten(ref, T, ts->labels, order.data(), lo.data(), hi.data(), edge.data(), program.data(), nullptr))
    return false;
  pllhip_ts_plan_splits(T, order.data(), lo.data(), hi.data(), words.data(), hash.data());
  pllhip_ts_sort_splits(T, R, words.data(), perm.data());
  out.words.resize((size_t)R * len);
  out.hash.resize(R);
  out.edge.resize(R);
  for (unsigned i = 0; i < R; ++i)
  {
    memcpy(out.words.data() + (size_t)i * len, words.data() + (size_t)perm[i] * len, (size_t)len * 4u);
    out.hash[i] = hash[perm[i]];
    out.edge[i] = edge[perm[i]];
  }
  return true;
}

// ids of the reference's splits on the device
bool lookup_reference(pllhip_treeset * ts, Job & j, const Reference & ref, unsigned ** d_ref_id)
{
  uint32_t * d_vec = nullptr;
  unsigned long long * d_hash = nullptr;
  if (!j.temp(&d_vec, ref.words.size(), "reference splits") || !j.temp(&d_hash, ts->R, "reference hashes") ||
      !j.temp(d_ref_id, ts->R, "reference ids"))
    return false;
  if (!j.start() || !j.up(d_vec, ref.words.data(), ref.words.size() * 4u) || !j.up(d_hash, ref.hash.data(), (size_t)ts->R * 8u) ||
      !j.stop(0, "uploading the reference"))
    return false;
  if (!j.start()) return false;
  hipLaunchKernelGGL(k_ts_lookup, dim3(grid_for(ts->R, TS_WG)), dim3(TS_WG), 0, j.stream, (const uint32_t *)d_vec,
                     (const unsigned long long *)d_hash, (const uint32_t *)ts->d_store, ts->len, ts->R,
                     hash_keep_mask(SPLIT_HASH_BITS), (const unsigned long long *)ts->d_table, (unsigned)(ts->slots - 1u),
                     *d_ref_id);
  return j.stop(1, "reference lookup");
}

// room for `need` entries, doubling: a set grows one tree at a time
template <typename V>
void room(V & v, size_t need)
{
  if (v.capacity() < need) v.reserve(std::max(need, 2u * v.capacity()));
}

bool check_set(const pllhip_treeset * ts, const void * a, const void * b, const char * who)
{
  if (!ts || !a || !b)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", who);
    return false;
  }
  if (!ts->count)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: the tree set is empty", who);
    return false;
  }
  return true;
}

// PLLHIP_CONSENSUS_BLOCK=<1..2048>: candidates per round of the greedy selection (a test knob; no result changes)
unsigned consensus_block()
{
  const char * env = getenv("PLLHIP_CONSENSUS_BLOCK");
  const long k = env && *env ? atol(env) : 1024L;
  return (unsigned)std::max(1L, std::min(k, (long)CS_MAX_BLOCK));
}

struct Consensus
{
  unsigned count = 0;
  std::vector<uint32_t> words;                                 // [count][len], in rank order
  std::vector<unsigned> trees;                                 // [count]
  unsigned long long tests[2] = {0, 0};
};

// the consensus split system of the set: ranking and selection on the device (kernels_treeset.hpp, k_cs_*)
bool run_consensus(pllhip_treeset * ts, double threshold, const char * who, Consensus & out)
{
  if (!ts)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", who);
    return false;
  }
  if (!(threshold >= 0.0 && threshold <= 1.0))
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: threshold %g is outside [0, 1]", who, threshold);
    return false;
  }
  if (!ts->count)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: the tree set is empty", who);
    return false;
  }
  unsigned need_major = 0, need_minor = 0;
  if (!pllhip_ts_consensus_needs(ts->count, threshold, &need_major, &need_minor)) return false;
  const unsigned T = ts->T, R = ts->R, len = ts->len;
  unsigned G = 1;
  while (G < len && G < 64u) G <<= 1;
  const unsigned block = consensus_block(), rowwords_max = (block + 31u) / 32u;

  Job j;
  if (!j.open(ts)) return false;
  if (!sync_cache(ts, j)) { drop_cache(ts); return false; }
  const unsigned D = ts->ndistinct;
  size_t cap = 1;
  while (cap < D) cap <<= 1;
  CsEntry * d_rank = nullptr;
  unsigned * d_state = nullptr, * d_acc_trees = nullptr, * d_survives = nullptr;
  unsigned long long * d_tests = nullptr;
  uint32_t * d_accepted = nullptr, * d_conflict = nullptr;
  unsigned state[4] = {0, 0, 0, 0};
  bool ok = j.temp(&d_rank, cap, "the ranked candidates") && j.temp(&d_state, 4, "consensus state") &&
            j.temp(&d_tests, 2, "consensus counters") && j.temp(&d_accepted, (size_t)R * len, "accepted splits") &&
            j.temp(&d_acc_trees, R, "accepted counts") && j.temp(&d_survives, block, "survivors") &&
            j.temp(&d_conflict, (size_t)block * rowwords_max, "the conflict matrix");
  ok = ok && j.start() && hip_ok(hipMemsetAsync(d_state, 0, 4 * sizeof(unsigned), j.stream), "memset") &&
       hip_ok(hipMemsetAsync(d_tests, 0, 2 * sizeof(unsigned long long), j.stream), "memset");
  if (!ok) { drop_cache(ts); return false; }
  hipLaunchKernelGGL(k_cs_candidates, dim3(grid_for(D, TS_WG)), dim3(TS_WG), 0, j.stream, (const unsigned *)ts->d_trees_with,
                     (const uint32_t *)ts->d_store, len, D, need_major, need_minor, d_rank, d_state);
  if (!j.down(state, d_state, sizeof(state)) || !j.stop(1, "consensus candidates")) { drop_cache(ts); return false; }
  const unsigned ncand = state[CS_NCAND], nmajor = state[CS_NMAJOR];
  if (ncand > D || nmajor > R || nmajor > ncand)
  {
    set_error(PLL_ERROR_HIP_RUNTIME, "%s: %u candidates of %u splits, %u of them in a majority of trees; a tree has %u",
              who, ncand, D, nmajor, R);
    drop_cache(ts);
    return false;
  }
  unsigned n = 1;
  while (n < ncand) n <<= 1;

  if (!j.start()) { drop_cache(ts); return false; }
  hipLaunchKernelGGL(k_cs_pad, dim3(grid_for(n - ncand, TS_WG)), dim3(TS_WG), 0, j.stream, d_rank, (const unsigned *)d_state, n);
  {
    const unsigned tiles = grid_for(n, 2u * TS_WG);
    const uint32_t * store = ts->d_store;
    hipLaunchKernelGGL(k_cs_sort_local, dim3(tiles), dim3(TS_WG), 0, j.stream, d_rank, n, 2u, std::min(n, 2u * TS_WG), store, len);
    for (unsigned k = 4u * TS_WG; k <= n && k; k <<= 1)
    {
      for (unsigned step = k >> 1; step > TS_WG; step >>= 1)
        hipLaunchKernelGGL(k_cs_sort_step, dim3(grid_for(n, TS_WG)), dim3(TS_WG), 0, j.stream, d_rank, n, k, step, store, len);
      hipLaunchKernelGGL(k_cs_sort_local, dim3(tiles), dim3(TS_WG), 0, j.stream, d_rank, n, k, k, store, len);
    }
  }
  hipLaunchKernelGGL(k_cs_take_majority, dim3(grid_for((size_t)nmajor * len, TS_WG)), dim3(TS_WG), 0, j.stream,
                     (const CsEntry *)d_rank, (const uint32_t *)ts->d_store, (const unsigned *)ts->d_trees_with, len, R,
                     d_accepted, d_acc_trees, d_state);
  unsigned held = nmajor;
  if (threshold < 0.5)
  {
    // the selection stops by itself once R splits are held (the kernels return at once); the host looks now and then
    unsigned rounds = 0;
    for (unsigned first = nmajor; first < ncand && held < R; first += block)
    {
      const unsigned nb = std::min(block, ncand - first), rowwords = (nb + 31u) / 32u;
      hipLaunchKernelGGL(k_cs_filter, dim3(grid_for(nb, 4)), dim3(TS_WG), 0, j.stream, (const CsEntry *)d_rank, first, nb,
                         (const uint32_t *)ts->d_store, (const uint32_t *)d_accepted, len, T, R, G, (const unsigned *)d_state,
                         d_survives, d_tests);
      hipLaunchKernelGGL(k_cs_pairs, dim3(grid_for(nb, 4)), dim3(TS_WG), 0, j.stream, (const CsEntry *)d_rank, first, nb,
                         (const uint32_t *)ts->d_store, len, T, R, G, (const unsigned *)d_state, (const unsigned *)d_survives,
                         d_conflict, rowwords, d_tests + 1);
      hipLaunchKernelGGL(k_cs_resolve, dim3(1), dim3(TS_WG), 0, j.stream, (const CsEntry *)d_rank, first, nb,
                         (const uint32_t *)ts->d_store, (const unsigned *)ts->d_trees_with, len, R, (const unsigned *)d_survives,
                         (const uint32_t *)d_conflict, rowwords, d_accepted, d_acc_trees, d_state);
      if (++rounds % 8u == 0u)
      {
        if (!j.down(state, d_state, sizeof(state)) || !hip_ok(hipStreamSynchronize(j.stream), "consensus selection"))
        { drop_cache(ts); return false; }
        held = state[CS_HELD];
      }
    }
  }
  if (!j.down(state, d_state, sizeof(state)) || !j.stop(1, "consensus kernels")) { drop_cache(ts); return false; }
  held = state[CS_HELD];
  if (held > R)
  {
    set_error(PLL_ERROR_HIP_RUNTIME, "%s: %u splits held, a tree has %u", who, held, R);
    drop_cache(ts);
    return false;
  }
  out.count = held;
  out.words.assign((size_t)held * len, 0u);
  out.trees.assign(held, 0u);
  if (!j.start() || (held && (!j.down(out.words.data(), d_accepted, (size_t)held * len * 4u) ||
                              !j.down(out.trees.data(), d_acc_trees, (size_t)held * sizeof(unsigned)))) ||
      !j.down(out.tests, d_tests, sizeof(out.tests)) || !j.stop(2, "download"))
  { drop_cache(ts); return false; }
  j.commit();
  g_last_consensus[0] = out.tests[0];
  g_last_consensus[1] = out.tests[1];
  return true;
}

} // namespace

extern "C" {

PLL_EXPORT pllhip_treeset_t * pllhip_treeset_create(unsigned int tip_count, const char * const * labels)
{
  if (tip_count < 4u || tip_count > PLLHIP_TS_MAX_TIPS)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_treeset_create: %u tips; 4 .. %u are supported", tip_count, PLLHIP_TS_MAX_TIPS);
    return nullptr;
  }
  pllhip_treeset * ts = new (std::nothrow) pllhip_treeset;
  if (!ts)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "pllhip_treeset_create: out of memory");
    return nullptr;
  }
  if (labels && !(ts->labels = pllhip_ts_labels_create(tip_count, labels)))
  {
    delete ts;
    return nullptr;
  }
  ts->T = tip_count;
  ts->len = pllhip_ts_words(tip_count);
  ts->R = tip_count - 3u;
  ts->stride = 1;
  while (ts->stride < ts->R) ts->stride <<= 1;
  ts->nsteps = (2u * tip_count - 3u + TS_CHUNK - 1u) / TS_CHUNK * TS_CHUNK;
  return ts;
}

PLL_EXPORT void pllhip_treeset_destroy(pllhip_treeset_t * ts)
{
  if (!ts) return;
  drop_cache(ts);
  pllhip_ts_labels_destroy(ts->labels);
  delete ts;
}

PLL_EXPORT unsigned int pllhip_treeset_count(const pllhip_treeset_t * ts)
{
  return ts ? ts->count : 0u;
}

PLL_EXPORT int pllhip_treeset_add(pllhip_treeset_t * ts, const pll_utree_t * tree)
{
  if (!ts || !tree)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_treeset_add: NULL argument");
    return PLL_FAILURE;
  }
  const unsigned T = ts->T, R = ts->R;
  try
  {
    std::vector<uint32_t> order(T - 1u), lo(R), hi(R);
    std::vector<pllhip_ts_step_t> program(2u * T - 3u);
    unsigned deepest = 0;
    if (!pllhip_ts_flatten(tree, T, ts->labels, order.data(), lo.data(), hi.data(), nullptr, program.data(), &deepest))
      return PLL_FAILURE;
    const size_t B = ts->count;
    room(ts->order, (B + 1u) * (T - 1u));
    room(ts->lohi, (B + 1u) * R);
    room(ts->program, (B + 1u) * ts->nsteps);
    room(ts->max_stack, B + 1u);
    // nothing throws from here on
    for (unsigned k = 0; k + 1u < T; ++k) ts->order.push_back((uint16_t)order[k]);
    for (unsigned e = 0; e < R; ++e) ts->lohi.push_back(lo[e] | (hi[e] << 16));
    for (unsigned s = 0; s < ts->nsteps; ++s)
      ts->program.push_back(s < 2u * T - 3u ? make_uint2(program[s].kind, program[s].arg) : make_uint2(TS_NOP, 0u));
    ts->max_stack.push_back(deepest);
    ts->count += 1u;
  }
  catch (const std::bad_alloc &)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "pllhip_treeset_add: out of memory");
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

PLL_EXPORT int pllhip_treeset_plan(const pllhip_treeset_t * ts, unsigned int index, unsigned int * order,
                                   unsigned int * lo, unsigned int * hi, unsigned int * program,
                                   unsigned int * max_stack)
{
  if (!ts || index >= ts->count)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_treeset_plan: NULL set or no tree %u", index);
    return PLL_FAILURE;
  }
  const unsigned T = ts->T, R = ts->R;
  for (unsigned k = 0; order && k + 1u < T; ++k) order[k] = ts->order[(size_t)index * (T - 1u) + k];
  for (unsigned e = 0; e < R; ++e)
  {
    const uint32_t iv = ts->lohi[(size_t)index * R + e];
    if (lo) lo[e] = iv & 0xffffu;
    if (hi) hi[e] = iv >> 16;
  }
  for (unsigned s = 0; program && s < 2u * T - 3u; ++s)
  {
    program[2u * s] = ts->program[(size_t)index * ts->nsteps + s].x;
    program[2u * s + 1u] = ts->program[(size_t)index * ts->nsteps + s].y;
  }
  if (max_stack) *max_stack = ts->max_stack[index];
  return PLL_SUCCESS;
}

PLL_EXPORT int pllhip_treeset_splits(pllhip_treeset_t * ts, unsigned int index, unsigned int * out)
{
  if (!check_set(ts, out, out, "pllhip_treeset_splits")) return PLL_FAILURE;
  if (index >= ts->count)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_treeset_splits: no tree %u in a set of %u", index, ts->count);
    return PLL_FAILURE;
  }
  const unsigned R = ts->R, len = ts->len;
  std::vector<uint32_t> words((size_t)R * len), perm(R);
  {
    Job j;
    uint32_t * d_out = nullptr;
    if (!j.open(ts)) return PLL_FAILURE;
    if (!sync_cache(ts, j) || !j.temp(&d_out, words.size(), "one tree's splits") || !j.start())
    { drop_cache(ts); return PLL_FAILURE; }
    hipLaunchKernelGGL(k_ts_gather, dim3(grid_for(words.size(), TS_WG)), dim3(TS_WG), 0, j.stream,
                       (const unsigned *)(ts->d_ids + (size_t)index * ts->stride), (const uint32_t *)ts->d_store, len, R, d_out);
    if (!j.stop(1, "split gather") || !j.start() || !j.down(words.data(), d_out, words.size() * 4u) || !j.stop(2, "download"))
    { drop_cache(ts); return PLL_FAILURE; }
    j.commit();
  }
  // ids are no order: the contract's order is by content
  pllhip_ts_sort_splits(ts->T, R, words.data(), perm.data());
  for (unsigned i = 0; i < R; ++i) memcpy(out + (size_t)i * len, words.data() + (size_t)perm[i] * len, (size_t)len * 4u);
  return PLL_SUCCESS;
}

PLL_EXPORT int pllhip_treeset_rf_matrix(pllhip_treeset_t * ts, unsigned int * out)
{
  if (!check_set(ts, out, out, "pllhip_treeset_rf_matrix")) return PLL_FAILURE;
  Job j;
  unsigned * d_out = nullptr;
  if (!j.open(ts)) return PLL_FAILURE;
  const size_t B = ts->count;
  std::vector<unsigned> host(B * B);
  if (!sync_cache(ts, j) || !j.temp(&d_out, B * B, "the RF matrix") || !j.start() ||
      !hip_ok(hipMemsetAsync(d_out, 0, B * B * sizeof(unsigned), j.stream), "memset"))
  { drop_cache(ts); return PLL_FAILURE; }
  hipLaunchKernelGGL(k_ts_rf_matrix, dim3(grid_for(B, 4), (unsigned)std::min<size_t>(B, 1024)), dim3(TS_WG), 0, j.stream,
                     (const unsigned *)ts->d_ids, ts->stride, ts->R, (unsigned)B, d_out);
  if (!j.stop(1, "RF kernel") || !j.start() || !j.down(host.data(), d_out, B * B * sizeof(unsigned)) || !j.stop(2, "download"))
  { drop_cache(ts); return PLL_FAILURE; }
  j.commit();
  memcpy(out, host.data(), B * B * sizeof(unsigned));
  return PLL_SUCCESS;
}

PLL_EXPORT int pllhip_treeset_rf_to(pllhip_treeset_t * ts, const pll_utree_t * ref, unsigned int * out)
{
  if (!check_set(ts, ref, out, "pllhip_treeset_rf_to")) return PLL_FAILURE;
  Reference r;
  if (!flatten_reference(ts, ref, r)) return PLL_FAILURE;
  Job j;
  unsigned * d_ref_id = nullptr, * d_out = nullptr;
  if (!j.open(ts)) return PLL_FAILURE;
  const unsigned B = ts->count;
  std::vector<unsigned> host(B);
  if (!sync_cache(ts, j) || !lookup_reference(ts, j, r, &d_ref_id) || !j.temp(&d_out, B, "RF distances") || !j.start())
  { drop_cache(ts); return PLL_FAILURE; }
  hipLaunchKernelGGL(k_ts_rf_to, dim3(grid_for(B, 4)), dim3(TS_WG), 0, j.stream, (const unsigned *)d_ref_id,
                     (const unsigned *)ts->d_ids, ts->stride, ts->R, B, d_out);
  if (!j.stop(1, "RF kernel") || !j.start() || !j.down(host.data(), d_out, (size_t)B * sizeof(unsigned)) || !j.stop(2, "download"))
  { drop_cache(ts); return PLL_FAILURE; }
  j.commit();
  memcpy(out, host.data(), (size_t)B * sizeof(unsigned));
  return PLL_SUCCESS;
}

PLL_EXPORT int pllhip_treeset_support(pllhip_treeset_t * ts, const pll_utree_t * ref, int kind, double * support,
                                      pll_unode_t ** split_to_node_map)
{
  if (!check_set(ts, ref, support, "pllhip_treeset_support")) return PLL_FAILURE;
  if (kind != PLLHIP_SUPPORT_FBP && kind != PLLHIP_SUPPORT_TBE)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_treeset_support: kind %d is neither PLLHIP_SUPPORT_FBP nor PLLHIP_SUPPORT_TBE", kind);
    return PLL_FAILURE;
  }
  Reference r;
  if (!flatten_reference(ts, ref, r)) return PLL_FAILURE;
  const unsigned T = ts->T, R = ts->R, len = ts->len, B = ts->count, groups = (R + 63u) / 64u;
  std::vector<unsigned long long> sums(R);
  std::vector<uint16_t> ones(R);
  for (unsigned i = 0; i < R; ++i)
  {
    unsigned p = 0;
    for (unsigned w = 0; w < len; ++w) p += (unsigned)__builtin_popcount(r.words[(size_t)i * len + w]);
    ones[i] = (uint16_t)p;
  }
  {
    Job j;
    unsigned long long * d_sums = nullptr;
    if (!j.open(ts)) return PLL_FAILURE;
    if (!sync_cache(ts, j) || !j.temp(&d_sums, R, "support sums")) { drop_cache(ts); return PLL_FAILURE; }
    if (kind == PLLHIP_SUPPORT_FBP)
    {
      unsigned * d_ref_id = nullptr;
      if (!lookup_reference(ts, j, r, &d_ref_id) || !j.start()) { drop_cache(ts); return PLL_FAILURE; }
      hipLaunchKernelGGL(k_ts_fbp, dim3(grid_for(R, TS_WG)), dim3(TS_WG), 0, j.stream, (const unsigned *)d_ref_id,
                         (const unsigned *)ts->d_trees_with, R, d_sums);
    }
    else
    {
      // the reference splits transposed: [tip][group of 64 splits]
      std::vector<unsigned long long> bits((size_t)T * groups, 0ULL);
      for (unsigned i = 0; i < R; ++i)
        for (unsigned w = 0; w < len; ++w)
          for (uint32_t m = r.words[(size_t)i * len + w]; m; m &= m - 1u)
            bits[(size_t)(32u * w + (unsigned)__builtin_ctz(m)) * groups + i / 64u] |= 1ULL << (i % 64u);
      unsigned long long * d_bits = nullptr;
      uint16_t * d_ones = nullptr;
      if (!j.temp(&d_bits, bits.size(), "transposed reference splits") || !j.temp(&d_ones, R, "split sizes") || !j.start() ||
          !j.up(d_bits, bits.data(), bits.size() * 8u) || !j.up(d_ones, ones.data(), (size_t)R * 2u) ||
          !hip_ok(hipMemsetAsync(d_sums, 0, (size_t)R * 8u, j.stream), "memset") || !j.stop(0, "uploading the reference") ||
          !j.start())
      { drop_cache(ts); return PLL_FAILURE; }
      const unsigned gx = (groups + 3u) / 4u;
      const unsigned gy = std::max(1u, std::min(B, std::max(1u, 8192u / gx)));
      hipLaunchKernelGGL(k_ts_tbe, dim3(gx, gy), dim3(TS_WG), 0, j.stream, (const uint2 *)ts->d_program, ts->nsteps,
                         (const unsigned long long *)d_bits, groups, (const uint16_t *)d_ones, R, T, B, d_sums);
    }
    if (!j.stop(1, "support kernel") || !j.start() || !j.down(sums.data(), d_sums, (size_t)R * 8u) || !j.stop(2, "download"))
    { drop_cache(ts); return PLL_FAILURE; }
    j.commit();
  }
  // the one division per split
  for (unsigned i = 0; i < R; ++i)
  {
    if (kind == PLLHIP_SUPPORT_FBP) support[i] = (double)sums[i] / (double)B;
    else
    {
      const unsigned p = std::min<unsigned>(ones[i], T - ones[i]);
      const unsigned long long den = (unsigned long long)B * (p - 1u);
      support[i] = (double)(den - sums[i]) / (double)den;
    }
    if (split_to_node_map) split_to_node_map[i] = r.edge[i];
  }
  g_last_sums = sums;
  return PLL_SUCCESS;
}

PLL_EXPORT int pllhip_treeset_consensus(pllhip_treeset_t * ts, double threshold, unsigned int * out_count,
                                        unsigned int * out_words, unsigned int * out_trees, double * out_support)
{
  try
  {
    Consensus c;
    if (!run_consensus(ts, threshold, "pllhip_treeset_consensus", c)) return PLL_FAILURE;
    if (out_count) *out_count = c.count;
    if (out_words && c.count) memcpy(out_words, c.words.data(), c.words.size() * 4u);
    for (unsigned i = 0; i < c.count; ++i)
    {
      if (out_trees) out_trees[i] = c.trees[i];
      if (out_support) out_support[i] = (double)c.trees[i] / (double)ts->count;      // the one division per split
    }
    return PLL_SUCCESS;
  }
  catch (const std::bad_alloc &)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "pllhip_treeset_consensus: out of memory");
    return PLL_FAILURE;
  }
}

PLL_EXPORT pll_utree_t * pllhip_treeset_tree_from_splits(const pllhip_treeset_t * ts, unsigned int count,
                                                         const unsigned int * words, const double * support)
{
  if (!ts)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_treeset_tree_from_splits: NULL argument");
    return nullptr;
  }
  return pllhip_ts_tree_from_splits(ts->T, ts->labels, count, words, support);
}

PLL_EXPORT pll_utree_t * pllhip_treeset_consensus_tree(pllhip_treeset_t * ts, double threshold)
{
  try
  {
    Consensus c;
    if (!run_consensus(ts, threshold, "pllhip_treeset_consensus_tree", c)) return nullptr;
    std::vector<double> support(c.count);
    for (unsigned i = 0; i < c.count; ++i) support[i] = (double)c.trees[i] / (double)ts->count;
    return pllhip_ts_tree_from_splits(ts->T, ts->labels, c.count, c.words.data(), support.data());
  }
  catch (const std::bad_alloc &)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "pllhip_treeset_consensus_tree: out of memory");
    return nullptr;
  }
}

PLL_EXPORT int pllhip_consensus_needs(unsigned int tree_count, double threshold, unsigned int * need_major,
                                      unsigned int * need_minor)
{
  return pllhip_ts_consensus_needs(tree_count, threshold, need_major, need_minor);
}

PLL_EXPORT void pllhip_treeset_last_consensus_counts(unsigned long long * accepted_tests, unsigned long long * pair_tests)
{
  if (accepted_tests) *accepted_tests = g_last_consensus[0];
  if (pair_tests) *pair_tests = g_last_consensus[1];
}

PLL_EXPORT unsigned int pllhip_treeset_last_sums(unsigned long long * out, unsigned int count)
{
  const unsigned n = (unsigned)std::min<size_t>(count, g_last_sums.size());
  for (unsigned i = 0; out && i < n; ++i) out[i] = g_last_sums[i];
  return (unsigned)g_last_sums.size();
}

PLL_EXPORT void pllhip_treeset_last_times(double * upload_ms, double * kernel_ms, double * download_ms)
{
  if (upload_ms) *upload_ms = g_last_ms[0];
  if (kernel_ms) *kernel_ms = g_last_ms[1];
  if (download_ms) *download_ms = g_last_ms[2];
}

PLL_EXPORT void pllhip_treeset_last_counts(unsigned long long * probe_steps, unsigned long long * compares)
{
  if (probe_steps) *probe_steps = g_last_counts[0];
  if (compares) *compares = g_last_counts[1];
}

}
