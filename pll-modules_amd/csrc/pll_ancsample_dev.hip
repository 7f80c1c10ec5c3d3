// pll_ancsample_dev.hip -- one coherent draw of all ancestral states from their joint posterior, given the data
// (kernels_ancsample.hpp, sim_plan.hpp; contract: INTEGRATION.md, "Sampled ancestral states"; design: DESIGN.md
// section 32).
//
// A call plans the edge list on the host (simplan::build, unchanged), has the engine store whatever vector exists as
// its operation or class table only, forms the site-category table of the root edge into planes of its own
// (sitecat_edge_table) and then walks the output in chunks of replicates -- or, where one replicate does not fit, of
// site ranges -- through two halves of a device staging buffer, as the simulation does: k_ancsample_walk fills one half
// on the partition's stream while a stream of the call's own copies the other to pinned memory.
#include "device_job.hpp"
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

constexpr unsigned ANCS_TILE = 256;                  // sites of a workgroup (kernels_ancsample.hpp, ANCS_WG)
constexpr unsigned ANCS_GROUP = 8;                   // replicates of a pass, at most (ANCS_RC)
constexpr unsigned ANCS_NONE = ~0u;
constexpr unsigned ANCS_MAX_STATES = 256, ANCS_MAX_CATS = 128;
constexpr u64 ANCS_DEFAULT_STAGING = 1ULL << 30;
constexpr u64 ANCS_MAX_ITEMS = 1ULL << 30;           // (tile, group) pairs of a launch

thread_local double g_ancs_ms[3] = {0.0, 0.0, 0.0};  // table, kernel, copy
thread_local u64 g_ancs_chunks = 0;

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

struct Chunk { unsigned rep0, reps, col0, cols; size_t pitch; };

bool invalid(const char * who, const std::string & what)
{
  set_error(PLL_ERROR_PARAM_INVALID, "%s: %s", who, what.c_str());
  return false;
}

} // namespace

// The draw behind pllhip_sample_ancestral_edges.  With a hook (device_job.hpp, AncsStageHook) every staging half holds
// state indices in all rows, tips included, the component row and the hook's extra rows, and the hook works on it on
// the partition's stream before it is copied out; the caller's rows, flags and alphabet are served on the host, so
// that `out` and `component` (either may then be NULL) hold what the call without a hook returns.
int pllhip::ancsample_run(const char * who, pll_partition_t * partition, const pllhip_ancsample_params_t * params,
                          unsigned int root_node, int root_scaler, unsigned int other_node, int other_scaler,
                          unsigned int edge_count, const unsigned int * parent, const unsigned int * child,
                          const unsigned int * matrix_indices, const unsigned int * freqs_indices,
                          unsigned int node_count, unsigned char * out, unsigned char * component,
                          unsigned long long * dropped, AncsStageHook * hook, double * times_ms)
{
  if (!partition || !partition->engine || !params || !freqs_indices || (!out && !hook))
    return invalid(who, "the partition, the parameters, freqs_indices or the output is NULL");
  if (edge_count && (!parent || !child || !matrix_indices)) return invalid(who, "the edge list is NULL");
  const unsigned known = PLLHIP_ANCS_TIPS | PLLHIP_ANCS_COMPONENT | (hook ? hook->flags : 0u);
  if (params->flags & ~known) return invalid(who, "unknown flags");
  const bool ask_tips = (params->flags & PLLHIP_ANCS_TIPS) != 0, ask_comp = (params->flags & PLLHIP_ANCS_COMPONENT) != 0;
  const bool with_tips = ask_tips || hook, with_comp = ask_comp || hook;
  if (ask_comp && !component) return invalid(who, "PLLHIP_ANCS_COMPONENT without a component array");
  if (!params->replicates) return invalid(who, "replicates is 0");
  if ((u64)params->first_replicate + params->replicates > (1ULL << 32))
    return invalid(who, "first_replicate + replicates exceeds 2^32");
  Engine * e = engine_of(partition);
  if (!e->shards.empty()) return invalid(who, "sharded partitions are not supported");
  const unsigned S = e->S, R = e->R, tips = partition->tips, N = e->Nreal;
  if (S > ANCS_MAX_STATES) return invalid(who, "more than 256 states do not fit the bytes of the output");
  if (R > ANCS_MAX_CATS) return invalid(who, "more than 128 categories do not fit the component byte");
  if (params->alphabet && strnlen(params->alphabet, S) < S)
    return invalid(who, "the alphabet has fewer than " + std::to_string(S) + " characters");
  bool pinv = false;
  for (unsigned r = 0; r < R; ++r)
  {
    if (freqs_indices[r] >= partition->rate_matrices)
      return invalid(who, "parameter index " + std::to_string(freqs_indices[r]) + " of category " + std::to_string(r) +
                          " out of range (" + std::to_string(partition->rate_matrices) + " rate matrices)");
    pinv = pinv || partition->prop_invar[freqs_indices[r]] > 0.0;
  }
  if (root_node >= node_count || other_node >= node_count)
    return invalid(who, "root edge node " + std::to_string(root_node >= node_count ? root_node : other_node) +
                        " out of range (" + std::to_string(node_count) + " nodes)");
  if (root_node < tips) return invalid(who, "root node " + std::to_string(root_node) + " is a tip");

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
  unsigned root_edges = 0, m0 = 0;
  for (const simplan::Step & s : plan.steps)
    if (s.parent == root_node && s.child == other_node) { ++root_edges; m0 = s.matrix; }
  if (root_edges != 1)
    return invalid(who, std::to_string(root_edges) + " edges lead from root node " + std::to_string(root_node) +
                        " to node " + std::to_string(other_node) + "; the list must hold the root edge once");
  if (!check_category_weights(partition->rate_weights, R, who)) return PLL_FAILURE;
  if (!N) { if (dropped) *dropped = 0; return PLL_SUCCESS; }

  const unsigned extra_row = node_count + 1u;        // the first row of the hook's own
  const unsigned rows = node_count + (with_comp ? 1u : 0u) + (hook ? hook->extra_rows : 0u);
  const unsigned comp_row = with_comp ? node_count : ANCS_NONE;
  auto row_of = [&](unsigned node) { return node >= tips || with_tips ? node : ANCS_NONE; };
  const size_t lds = (size_t)plan.slots * ANCS_TILE * sizeof(u64) + 256;
  if (lds > (64u << 10)) return invalid(who, "the tree needs more slots than the LDS of a workgroup holds");

  // chunks: whole replicates, or site ranges of one
  const u64 budget = env_u64("PLLHIP_ANCS_STAGING_BYTES", ANCS_DEFAULT_STAGING);
  const u64 half = std::max<u64>(budget / 2, (u64)rows * ANCS_TILE);
  const u64 per_pass = std::min<u64>(ANCS_GROUP, env_u64("PLLHIP_ANCS_REPLICATES", ANCS_GROUP));
  const u64 rep_cap = hook && hook->chunk_replicates ? hook->chunk_replicates : ~0ULL;
  const u64 sites = N, full_pitch = (sites + 3) & ~3ULL;
  u64 chunk_reps = 1, chunk_cols = sites;
  if ((u64)rows * full_pitch <= half)
  {
    const u64 tiles = (sites + ANCS_TILE - 1) / ANCS_TILE;
    chunk_reps = std::max<u64>(1, std::min<u64>({(u64)params->replicates, half / ((u64)rows * full_pitch),
                                                 ANCS_MAX_ITEMS / tiles, rep_cap}));
  }
  else
    chunk_cols = std::max<u64>(ANCS_TILE, half / rows / ANCS_TILE * ANCS_TILE);
  std::vector<Chunk> chunks;
  for (u64 r0 = 0; r0 < params->replicates; r0 += chunk_reps)
    for (u64 c0 = 0; c0 < sites; c0 += chunk_cols)
    {
      Chunk c;
      c.rep0 = (unsigned)r0;
      c.reps = (unsigned)std::min<u64>(chunk_reps, params->replicates - r0);
      c.col0 = (unsigned)c0;
      c.cols = (unsigned)std::min<u64>(chunk_cols, sites - c0);
      c.pitch = ((size_t)c.cols + 3) & ~(size_t)3;
      chunks.push_back(c);
    }
  const size_t half_bytes = (size_t)chunk_reps * rows * (((size_t)std::min<u64>(chunk_cols, sites) + 3) & ~(size_t)3);
  const unsigned nhalves = chunks.size() > 1 ? 2 : 1;
  const u64 block_cap = env_u64("PLLHIP_ANCS_BLOCKS", 0);

  DeviceJob j;
  CopyStream copy;
  if (!j.enter(e->device, e->stream) || !copy.open()) return PLL_FAILURE;

  // the vectors of the call: the root, then the child of every step
  std::vector<unsigned> nodes(1, root_node);
  for (const simplan::Step & s : plan.steps) nodes.push_back(s.child);
  std::vector<AncsVector> views(nodes.size());
  AncsOperands ops;
  if (!ancsample_operands(partition, freqs_indices, nodes.data(), (unsigned)nodes.size(), ops, views.data())) return PLL_FAILURE;
  const size_t pm_cells = (size_t)R * S * e->Sp;
  std::vector<AncsStep> steps(plan.steps.size());
  AncsVector other_view;
  for (size_t k = 0; k < steps.size(); ++k)
  {
    const simplan::Step & s = plan.steps[k];
    steps[k].child = views[k + 1];
    steps[k].pm = (u64)s.matrix * pm_cells;
    steps[k].stream = 3u + s.matrix;
    steps[k].src = s.src;
    steps[k].dst = s.dst == simplan::NONE ? ANCS_NONE : s.dst;
    steps[k].row = row_of(s.child);
    if (s.parent == root_node && s.child == other_node) other_view = views[k + 1];
  }

  // the tables of the call
  uint8_t h_alpha[256], h_ident[256];
  for (unsigned s = 0; s < 256; ++s) h_alpha[s] = (uint8_t)(params->alphabet && s < S ? params->alphabet[s] : s);
  for (unsigned s = 0; s < 256; ++s) h_ident[s] = (uint8_t)s;
  uint8_t h_lut[256];                                  // with a hook the host maps; 0xFF stays 0xFF, as in the kernel
  memcpy(h_lut, h_alpha, 256);
  h_lut[255] = 255;
  const size_t plane = ((size_t)N + 1) & ~(size_t)1;
  SiteCatPlanes planes;
  planes.A = j.alloc<double>((size_t)R * plane, "site-category table");
  planes.B = pinv ? j.alloc<double>((size_t)R * plane, "site-category table") : nullptr;
  planes.c = j.alloc<unsigned>(N, "site-category counts");
  planes.plane = plane;
  unsigned * d_m = j.alloc<unsigned>(N, "pattern weights");
  u64 * d_dropped = j.alloc<u64>(1, "dropped sites");
  AncsStep * d_steps = j.alloc<AncsStep>(steps.size(), "edge program");
  uint8_t * d_alpha = j.alloc<uint8_t>(256, "alphabet");
  uint8_t * d_half[2] = {nullptr, nullptr}, * h_half[2] = {nullptr, nullptr};
  hipEvent_t k0[2], k1[2], c0[2], c1[2], w1[2] = {nullptr, nullptr};
  bool ok = planes.A && (!pinv || planes.B) && planes.c && d_m && d_dropped && d_steps && d_alpha;
  for (unsigned h = 0; ok && h < nhalves; ++h)
  {
    d_half[h] = j.alloc<uint8_t>(half_bytes, "the staging buffer");
    h_half[h] = j.pinned<uint8_t>(half_bytes);
    k0[h] = j.event(); k1[h] = j.event(); c0[h] = j.event(); c1[h] = j.event();
    if (hook) w1[h] = j.event();
    ok = d_half[h] && h_half[h] && k0[h] && k1[h] && c0[h] && c1[h] && (!hook || w1[h]);
  }
  if (!ok) return PLL_FAILURE;
  // (pageable sources: the runtime stages them before it returns)
  if (!j.upload(d_steps, steps.data(), steps.size(), "upload edge program") ||
      !j.upload(d_alpha, hook ? h_ident : h_alpha, 256, "upload alphabet") ||
      !j.upload(d_m, partition->pattern_weights, N, "upload pattern weights") ||
      !hip_ok(hipMemsetAsync(d_dropped, 0, sizeof(u64), j.stream), "hipMemsetAsync"))
    return PLL_FAILURE;
  hipEvent_t t0 = j.mark();
  if (!t0 || !sitecat_edge_table(partition, root_node, root_scaler, other_node, other_scaler, m0, freqs_indices, planes))
    return PLL_FAILURE;
  hipEvent_t t1 = j.mark();
  if (!t1) return PLL_FAILURE;
  if (hook && !hook->prepare(j, ops.cu_count, d_m)) return PLL_FAILURE;

  const size_t out_rows = node_count;
  double kernel_ms = 0.0, copy_ms = 0.0, hook_ms = 0.0;
  auto staged = [&](const Chunk & c, uint8_t * half) {
    AncsStaged s;
    s.half = half;
    s.rep0 = c.rep0; s.reps = c.reps; s.col0 = c.col0; s.cols = c.cols;
    s.rows = rows; s.comp_row = comp_row; s.extra_row = extra_row;
    s.pitch = c.pitch;
    return s;
  };

  // chunk q is in pinned half q & 1: wait for its copy, then put its rows where the caller wants them
  auto deliver = [&](size_t q) -> bool {
    const Chunk & c = chunks[q];
    const unsigned h = (unsigned)(q & 1);
    float km = 0.f, cm = 0.f;
    if (!hip_ok(hipEventSynchronize(c1[h]), "copy of a staging chunk") || !j.elapsed(k0[h], k1[h], &km) ||
        !j.elapsed(c0[h], c1[h], &cm))
      return false;
    if (hook)
    {
      float wm = 0.f;
      if (!j.elapsed(k0[h], w1[h], &wm)) return false;
      hook_ms += km - wm;
      km = wm;
    }
    kernel_ms += km;
    const auto begin = std::chrono::steady_clock::now();
    for (unsigned r = 0; r < c.reps; ++r)
    {
      const uint8_t * src = h_half[h] + (size_t)r * rows * c.pitch;
      for (size_t row = 0; out && row < out_rows; ++row)
      {
        uint8_t * dst = out + ((size_t)(c.rep0 + r) * out_rows + row) * sites + c.col0;
        if (!hook) memcpy(dst, src + row * c.pitch, c.cols);
        else if (row < tips && !ask_tips) memset(dst, 0xff, c.cols);
        else for (unsigned x = 0; x < c.cols; ++x) dst[x] = h_lut[src[row * c.pitch + x]];
      }
      if (ask_comp) memcpy(component + (size_t)(c.rep0 + r) * sites + c.col0, src + (size_t)comp_row * c.pitch, c.cols);
    }
    if (hook) hook->deliver(staged(c, h_half[h]));
    copy_ms += cm + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - begin).count();
    return true;
  };

  for (size_t q = 0; q < chunks.size(); ++q)
  {
    const Chunk & c = chunks[q];
    const unsigned h = (unsigned)(q & 1);
    if (q >= 2 && !deliver(q - 2)) return PLL_FAILURE;      // (so half h is free on the device and on the host)
    AncsLaunch L;
    L.steps = d_steps;
    L.nsteps = (unsigned)steps.size();
    L.slots = plan.slots;
    L.root = views[0];
    L.other = other_view;
    L.pm0 = (u64)m0 * pm_cells;
    L.root_row = row_of(root_node);
    L.A = planes.A;
    L.B = planes.B;
    L.plane = plane;
    L.m = d_m;
    L.dropped = c.rep0 == 0 ? d_dropped : nullptr;           // every site is in one such chunk
    L.seed = params->seed;
    L.first_replicate = params->first_replicate + c.rep0;
    L.replicates = c.reps;
    L.per_pass = (unsigned)per_pass;
    L.site0 = c.col0;
    L.sites = c.cols;
    L.tiles = (c.cols + ANCS_TILE - 1) / ANCS_TILE;
    L.rows = rows;
    L.comp_row = comp_row;
    L.pitch = c.pitch;
    L.out = d_half[h];
    L.alphabet = d_alpha;
    const u64 items = (u64)L.tiles * ((c.reps + per_pass - 1) / per_pass);
    const u64 wanted = std::min<u64>(items, (u64)ops.cu_count * 32);
    const unsigned grid = (unsigned)std::max<u64>(1, block_cap ? std::min(wanted, block_cap) : wanted);
    if (!hip_ok(hipEventRecord(k0[h], j.stream), "hipEventRecord") ||
        !hip_ok(hipMemsetAsync(d_half[h], 0xff, (size_t)c.reps * rows * c.pitch, j.stream), "hipMemsetAsync") ||
        !ancsample_walk(partition, ops, L, grid) ||
        (hook && (!hip_ok(hipEventRecord(w1[h], j.stream), "hipEventRecord") || !hook->launch(j, staged(c, d_half[h])))) ||
        !hip_ok(hipEventRecord(k1[h], j.stream), "hipEventRecord") ||
        !hip_ok(hipStreamWaitEvent(copy.s, k1[h], 0), "hipStreamWaitEvent") ||
        !hip_ok(hipEventRecord(c0[h], copy.s), "hipEventRecord") ||
        !hip_ok(hipMemcpyAsync(h_half[h], d_half[h], (size_t)c.reps * rows * c.pitch, hipMemcpyDeviceToHost, copy.s),
                "copy of a staging chunk") ||
        !hip_ok(hipEventRecord(c1[h], copy.s), "hipEventRecord"))
      return PLL_FAILURE;
  }
  for (size_t q = chunks.size() >= 2 ? chunks.size() - 2 : 0; q < chunks.size(); ++q)
    if (!deliver(q)) return PLL_FAILURE;
  u64 h_dropped = 0;
  float tm = 0.f;
  if (!j.download(&h_dropped, d_dropped, 1, "download") || !hip_ok(hipStreamSynchronize(j.stream), "download") ||
      !j.elapsed(t0, t1, &tm))
    return PLL_FAILURE;
  if (hook && !hook->finish(j)) return PLL_FAILURE;
  if (dropped) *dropped = h_dropped;
  if (times_ms)
  {
    times_ms[0] = tm; times_ms[1] = kernel_ms; times_ms[2] = hook_ms; times_ms[3] = copy_ms;
    return PLL_SUCCESS;
  }
  g_ancs_ms[0] = tm;
  g_ancs_ms[1] = kernel_ms;
  g_ancs_ms[2] = copy_ms;
  g_ancs_chunks = chunks.size();
  return PLL_SUCCESS;
}

extern "C" {

PLL_EXPORT int pllhip_sample_ancestral_edges(pll_partition_t * partition, const pllhip_ancsample_params_t * params,
                                             unsigned int root_node, int root_scaler, unsigned int other_node,
                                             int other_scaler, unsigned int edge_count, const unsigned int * parent,
                                             const unsigned int * child, const unsigned int * matrix_indices,
                                             const unsigned int * freqs_indices, unsigned int node_count,
                                             unsigned char * out, unsigned char * component, unsigned long long * dropped)
{
  return ancsample_run("pllhip_sample_ancestral_edges", partition, params, root_node, root_scaler, other_node,
                       other_scaler, edge_count, parent, child, matrix_indices, freqs_indices, node_count, out, component,
                       dropped, nullptr, nullptr);
}

PLL_EXPORT void pllhip_ancsample_last_times(double * table_ms, double * kernel_ms, double * copy_ms,
                                            unsigned long long * chunks)
{
  if (table_ms) *table_ms = g_ancs_ms[0];
  if (kernel_ms) *kernel_ms = g_ancs_ms[1];
  if (copy_ms) *copy_ms = g_ancs_ms[2];
  if (chunks) *chunks = g_ancs_chunks;
}

} // extern "C"
