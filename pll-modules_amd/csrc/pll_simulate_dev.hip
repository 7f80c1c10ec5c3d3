// pll_simulate_dev.hip -- alignments drawn from a partition's model along a tree (kernels_simulate.hpp, sim_plan.hpp;
// contract: INTEGRATION.md, "Simulated alignments"; design: DESIGN.md section 28).
//
// A call plans the edge list on the host, cumulates the matrices it uses once (k_sim_cumulate) and then walks the
// output in chunks of replicates -- or, where one replicate does not fit, of site ranges -- through two halves of a
// device staging buffer: k_sim_evolve fills one half on the partition's stream while a stream of the call's own copies
// the other to pinned memory, from where the host puts the rows into the caller's array.
#include "device_job.hpp"
#include "kernels_simulate.hpp"
#include "sim_plan.hpp"
#include "pllhip.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace pllhip;

namespace {

using u64 = unsigned long long;

constexpr u64 SIM_DEFAULT_STAGING = 1ULL << 30;
constexpr u64 SIM_MAX_CHUNK_SITES = 1ULL << 30;     // columns of a chunk (32-bit column numbers in the kernel)
constexpr u64 SIM_MAX_ITEMS = 1ULL << 30;           // (tile, replicate) pairs of a launch

thread_local double g_sim_ms[3] = {0.0, 0.0, 0.0};  // tables, kernel, copy
thread_local u64 g_sim_chunks = 0;

u64 env_u64(const char * name, u64 fallback)
{
  const char * v = getenv(name);
  if (!v || !*v) return fallback;
  const u64 x = strtoull(v, nullptr, 10);
  return x ? x : fallback;
}

// a second stream, for the copies out of the staging halves
struct CopyStream
{
  hipStream_t s = nullptr;
  ~CopyStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
  bool open() { return hip_ok(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate"); }
};

struct Chunk { unsigned rep0, reps; u64 col0; unsigned cols; size_t pitch; };

bool invalid(const char * who, const std::string & what)
{
  set_error(PLL_ERROR_PARAM_INVALID, "%s: %s", who, what.c_str());
  return false;
}

} // namespace

extern "C" {

PLL_EXPORT int pllhip_simulate_edges(pll_partition_t * partition, const pllhip_sim_params_t * params,
                                     unsigned int root_node, unsigned int edge_count, const unsigned int * parent,
                                     const unsigned int * child, const unsigned int * matrix_indices,
                                     const unsigned int * params_indices, unsigned int node_count, unsigned char * out)
{
  const char * who = "pllhip_simulate_edges";
  if (!partition || !partition->engine || !params || !params_indices || !out)
    return invalid(who, "the partition, the parameters, params_indices or the output is NULL");
  if (!params->sites || !params->replicates)
    return invalid(who, !params->sites ? "sites is 0" : "replicates is 0");
  if ((u64)params->first_replicate + params->replicates > (1ULL << 32))
    return invalid(who, "first_replicate + replicates exceeds 2^32");
  if (params->first_site + params->sites < params->first_site) return invalid(who, "first_site + sites exceeds 2^64");
  if (partition->attributes & (PLL_ATTRIB_AB_FLAG | PLL_ATTRIB_AB_MASK))
    return invalid(who, "the partition has an ascertainment-bias attribute; conditioning on variable sites is a "
                        "different process and is not simulated");
  Engine * e = exec_engine(partition);
  const unsigned S = e->S, R = e->R, tips = partition->tips;
  if (S > SIM_MAX_STATES) return invalid(who, "more than 256 states do not fit the bytes of the output");
  for (unsigned c = 0; c < R; ++c)
    if (params_indices[c] >= partition->rate_matrices)
      return invalid(who, "params index " + std::to_string(params_indices[c]) + " of category " + std::to_string(c) +
                          " out of range (" + std::to_string(partition->rate_matrices) + " rate matrices)");
  if (params->alphabet && strnlen(params->alphabet, S) < S)
    return invalid(who, "the alphabet has fewer than " + std::to_string(S) + " characters");
  if (params->flags & ~(unsigned)PLLHIP_SIM_INNER) return invalid(who, "unknown flags");

  simplan::Input in;
  in.tips = tips;
  in.node_count = node_count;
  in.matrix_count = partition->prob_matrices;
  in.root = root_node;
  in.edge_count = edge_count;
  in.parent = parent;
  in.child = child;
  in.matrix = matrix_indices;
  simplan::Plan plan;
  std::string error;
  if (!simplan::build(in, plan, error)) return invalid(who, error);

  const bool inner = (params->flags & PLLHIP_SIM_INNER) != 0;
  const unsigned rows = inner ? node_count : tips;
  auto row_of = [&](unsigned node) { return node < tips || inner ? node : SIM_NO; };
  std::vector<unsigned> table_of(partition->prob_matrices, 0);
  for (size_t t = 0; t < plan.matrices.size(); ++t) table_of[plan.matrices[t]] = (unsigned)t;
  std::vector<SimStep> steps(plan.steps.size());
  for (size_t k = 0; k < steps.size(); ++k)
  {
    const simplan::Step & s = plan.steps[k];
    steps[k].src = s.src;
    steps[k].dst = s.dst == simplan::NONE ? SIM_NO : s.dst;
    steps[k].table = table_of[s.matrix];
    steps[k].stream = 3u + s.matrix;
    steps[k].row = row_of(s.child);
  }
  const bool holes = inner && plan.nodes_reached < node_count;     // rows of nodes the list does not name: 0xFF

  // LDS of a workgroup: the slots and the alphabet, and the rows of one matrix where they fit beside them
  const size_t RSS = (size_t)R * S * S, nt = plan.matrices.size();
  const size_t lds_slots = (size_t)plan.slots * SIM_WG * sizeof(unsigned) + 256;
  if (lds_slots > SIM_LDS_BUDGET) return invalid(who, "the tree needs more slots than the LDS budget holds");
  const bool staged = RSS * sizeof(double) + lds_slots <= SIM_LDS_BUDGET;
  const size_t lds = lds_slots + (staged ? RSS * sizeof(double) : 0);

  // chunks: whole replicates, or site ranges of one
  const u64 budget = env_u64("PLLHIP_SIM_STAGING_BYTES", SIM_DEFAULT_STAGING);
  const u64 half = std::max<u64>(budget / 2, (u64)rows * SIM_TILE);
  const u64 sites = params->sites, full_pitch = (sites + 3) & ~3ULL;
  u64 chunk_reps = 1, chunk_cols = sites;
  if ((u64)rows * full_pitch <= half && sites <= SIM_MAX_CHUNK_SITES)
  {
    const u64 tiles = (sites + SIM_TILE - 1) / SIM_TILE;
    chunk_reps = std::min<u64>({(u64)params->replicates, half / ((u64)rows * full_pitch), SIM_MAX_ITEMS / tiles});
  }
  else
    chunk_cols = std::min<u64>(SIM_MAX_CHUNK_SITES, std::max<u64>(SIM_TILE, half / rows / SIM_TILE * SIM_TILE));
  std::vector<Chunk> chunks;
  for (u64 r0 = 0; r0 < params->replicates; r0 += chunk_reps)
    for (u64 c0 = 0; c0 < sites; c0 += chunk_cols)
    {
      Chunk c;
      c.rep0 = (unsigned)r0;
      c.reps = (unsigned)std::min<u64>(chunk_reps, params->replicates - r0);
      c.col0 = c0;
      c.cols = (unsigned)std::min<u64>(chunk_cols, sites - c0);
      c.pitch = ((size_t)c.cols + 3) & ~(size_t)3;
      chunks.push_back(c);
    }
  const size_t half_bytes = (size_t)chunk_reps * rows * (((size_t)std::min<u64>(chunk_cols, sites) + 3) & ~(size_t)3);
  const unsigned nhalves = chunks.size() > 1 ? 2 : 1;
  const u64 block_cap = env_u64("PLLHIP_SIM_BLOCKS", 0);

  DeviceJob j;
  CopyStream copy;
  pllhip::MatrixTables mt;
  if (!j.enter(e->device, e->stream) || !copy.open() || !matrix_tables(partition, mt)) return PLL_FAILURE;

  // the tables of the call
  uint8_t h_alpha[256];
  for (unsigned s = 0; s < 256; ++s) h_alpha[s] = (uint8_t)(params->alphabet && s < S ? params->alphabet[s] : s);
  ParamIdxHost pidx = {};
  for (unsigned c = 0; c < R; ++c) pidx.v[c] = params_indices[c];
  double * d_cum = j.alloc<double>(nt * RSS, "cumulated matrices");
  double * d_cumw = j.alloc<double>(R, "cumulated weights");
  double * d_cumf = j.alloc<double>((size_t)R * S, "cumulated frequencies");
  double * d_pinv = j.alloc<double>(R, "invariant proportions");
  unsigned * d_tables = j.alloc<unsigned>(nt, "matrix list");
  SimStep * d_steps = j.alloc<SimStep>(steps.size(), "edge program");
  uint8_t * d_alpha = j.alloc<uint8_t>(256, "alphabet");
  uint8_t * d_half[2] = {nullptr, nullptr}, * h_half[2] = {nullptr, nullptr};
  hipEvent_t k0[2], k1[2], c0[2], c1[2];
  bool ok = d_cum && d_cumw && d_cumf && d_pinv && d_tables && d_steps && d_alpha;
  for (unsigned h = 0; ok && h < nhalves; ++h)
  {
    d_half[h] = j.alloc<uint8_t>(half_bytes, "the staging buffer");
    h_half[h] = j.pinned<uint8_t>(half_bytes);
    k0[h] = j.event(); k1[h] = j.event(); c0[h] = j.event(); c1[h] = j.event();
    ok = d_half[h] && h_half[h] && k0[h] && k1[h] && c0[h] && c1[h];
  }
  if (!ok) return PLL_FAILURE;
  // (pageable sources: the runtime stages them before it returns)
  if (!j.upload(d_tables, plan.matrices.data(), nt, "upload matrix list") ||
      !j.upload(d_steps, steps.data(), steps.size(), "upload edge program") ||
      !j.upload(d_alpha, h_alpha, 256, "upload alphabet"))
    return PLL_FAILURE;
  hipEvent_t t0 = j.mark();
  hipLaunchKernelGGL(k_sim_cumulate, dim3(grid_for(nt * R * S + R + 1, SIM_WG)), dim3(SIM_WG), 0, j.stream,
                     mt.pmat, mt.model, mt.off_weights, mt.off_pinv, mt.off_freqs, d_tables, (unsigned)nt, pidx, R, S,
                     e->Sp, d_cum, d_cumw, d_cumf, d_pinv);
  hipEvent_t t1 = j.mark();
  if (!t0 || !t1 || !hip_ok(hipGetLastError(), "k_sim_cumulate")) return PLL_FAILURE;

  SimTables T;
  T.cum = d_cum;
  T.cumw = d_cumw;
  T.cumf = d_cumf;
  T.pinv = d_pinv;
  T.alphabet = d_alpha;
  double kernel_ms = 0.0, copy_ms = 0.0;

  // chunk q is in pinned half q & 1: wait for its copy, then put its rows where the caller wants them
  auto deliver = [&](size_t q) -> bool {
    const Chunk & c = chunks[q];
    const unsigned h = (unsigned)(q & 1);
    float km = 0.f, cm = 0.f;
    if (!hip_ok(hipEventSynchronize(c1[h]), "copy of a staging chunk") || !j.elapsed(k0[h], k1[h], &km) ||
        !j.elapsed(c0[h], c1[h], &cm))
      return false;
    kernel_ms += km;
    const auto begin = std::chrono::steady_clock::now();
    for (unsigned r = 0; r < c.reps; ++r)
      for (unsigned row = 0; row < rows; ++row)
        memcpy(out + ((size_t)(c.rep0 + r) * rows + row) * sites + c.col0, h_half[h] + ((size_t)r * rows + row) * c.pitch,
               c.cols);
    copy_ms += cm + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - begin).count();
    return true;
  };

  for (size_t q = 0; q < chunks.size(); ++q)
  {
    const Chunk & c = chunks[q];
    const unsigned h = (unsigned)(q & 1);
    if (q >= 2 && !deliver(q - 2)) return PLL_FAILURE;      // (so half h is free on the device and on the host)
    SimLaunch L;
    L.steps = d_steps;
    L.nsteps = (unsigned)steps.size();
    L.slots = plan.slots;
    L.root_row = row_of(root_node);
    L.R = R;
    L.S = S;
    L.seed = params->seed;
    L.first_site = params->first_site + c.col0;
    L.first_replicate = params->first_replicate + c.rep0;
    L.replicates = c.reps;
    L.sites = c.cols;
    L.tiles = (c.cols + SIM_TILE - 1) / SIM_TILE;
    L.rows = rows;
    L.pitch = c.pitch;
    L.out = d_half[h];
    const u64 items = (u64)L.tiles * L.replicates;
    const unsigned grid = (unsigned)(block_cap ? std::min(items, block_cap) : items);
    if (!hip_ok(hipEventRecord(k0[h], j.stream), "hipEventRecord")) return PLL_FAILURE;
    if (holes && !hip_ok(hipMemsetAsync(d_half[h], 0xff, (size_t)c.reps * rows * c.pitch, j.stream), "hipMemsetAsync"))
      return PLL_FAILURE;
    if (staged) hipLaunchKernelGGL(k_sim_evolve<true>, dim3(grid), dim3(SIM_WG), lds, j.stream, T, L);
    else hipLaunchKernelGGL(k_sim_evolve<false>, dim3(grid), dim3(SIM_WG), lds, j.stream, T, L);
    if (!hip_ok(hipGetLastError(), "k_sim_evolve") || !hip_ok(hipEventRecord(k1[h], j.stream), "hipEventRecord") ||
        !hip_ok(hipStreamWaitEvent(copy.s, k1[h], 0), "hipStreamWaitEvent") ||
        !hip_ok(hipEventRecord(c0[h], copy.s), "hipEventRecord") ||
        !hip_ok(hipMemcpyAsync(h_half[h], d_half[h], (size_t)c.reps * rows * c.pitch, hipMemcpyDeviceToHost, copy.s),
                "copy of a staging chunk") ||
        !hip_ok(hipEventRecord(c1[h], copy.s), "hipEventRecord"))
      return PLL_FAILURE;
  }
  for (size_t q = chunks.size() >= 2 ? chunks.size() - 2 : 0; q < chunks.size(); ++q)
    if (!deliver(q)) return PLL_FAILURE;
  float tm = 0.f;
  if (!j.elapsed(t0, t1, &tm)) return PLL_FAILURE;
  g_sim_ms[0] = tm;
  g_sim_ms[1] = kernel_ms;
  g_sim_ms[2] = copy_ms;
  g_sim_chunks = chunks.size();
  return PLL_SUCCESS;
}

PLL_EXPORT void pllhip_simulate_last_times(double * tables_ms, double * kernel_ms, double * copy_ms,
                                           unsigned long long * chunks)
{
  if (tables_ms) *tables_ms = g_sim_ms[0];
  if (kernel_ms) *kernel_ms = g_sim_ms[1];
  if (copy_ms) *copy_ms = g_sim_ms[2];
  if (chunks) *chunks = g_sim_chunks;
}

} // extern "C"
