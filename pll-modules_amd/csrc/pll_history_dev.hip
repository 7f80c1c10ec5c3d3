// pll_history_dev.hip -- sampled substitution histories: the ancestral draw of pll_ancsample_dev.hip with one more
// stage on every staging half (kernels_history.hpp; contract: INTEGRATION.md, "Sampled substitution histories";
// design: DESIGN.md section 33).
//
// The call builds the host tables (host/pllhip_history.h: the powers of the uniformized matrix per rate matrix, a
// Poisson table per edge and category), runs ancsample_run with a hook that uploads them once, launches
// k_history_edges on each half between the walk and the copy, takes the per-site rows out of the pinned copy and
// downloads the integer tables at the end.
#include "device_job.hpp"
#include "kernels_history.hpp"
#include "host/pllhip_history.h"
#include "pllhip.h"

#include <cstring>
#include <vector>

using namespace pllhip;

namespace {

using u64 = unsigned long long;

static_assert(HIST_STREAM == PLLHIP_HIST_STREAM, "one stream base on both sides");

constexpr unsigned HIST_LDS_STATES = 64;             // up to here a workgroup keeps its tables in LDS ...
constexpr size_t HIST_LDS_BYTES = 48u << 10;         // ... if they fit this

thread_local double g_hist_ms[4] = {0.0, 0.0, 0.0, 0.0};   // table, walk, history, copy

struct HistoryHook : AncsStageHook
{
  pll_partition_t * partition = nullptr;
  const pllhip_ancsample_params_t * params = nullptr;
  const pllhip_history_tables_t * T = nullptr;
  unsigned edges = 0, sites = 0;
  const unsigned * parent = nullptr, * child = nullptr, * matrix = nullptr;
  u64 * counts = nullptr, * units = nullptr, * dropped_edges = nullptr;      // the caller's
  unsigned char * changes = nullptr;

  HistLaunch L;
  unsigned cu = 0;
  size_t counts_cells = 0, units_cells = 0, edge_cells = 0;

  bool prepare(DeviceJob & j, unsigned cu_count, const unsigned * d_pattern_weights) override
  {
    const unsigned S = T->states, R = T->cats;
    cu = cu_count;
    counts_cells = (size_t)params->replicates * edges * S * S;
    units_cells = (size_t)params->replicates * edges * R * S;
    edge_cells = (size_t)params->replicates * edges;
    std::vector<HistEdge> list(edges);
    for (unsigned e = 0; e < edges; ++e)
    {
      list[e].parent_row = parent[e];
      list[e].child_row = child[e];
      list[e].matrix = matrix[e];
    }
    HistEdge * d_edge = j.alloc<HistEdge>(edges, "history edges");
    unsigned * d_slot = j.alloc<unsigned>(R, "history tables");
    double * d_rpow = j.alloc<double>((size_t)T->nmat * T->kmax * S * S, "powers of the uniformized matrix");
    unsigned * d_len = j.alloc<unsigned>((size_t)edges * R, "history tables");
    u64 * d_off = j.alloc<u64>((size_t)edges * R, "history tables");
    double * d_pois = j.alloc<double>(T->pois_count, "Poisson tables");
    L.counts = j.alloc<u64>(counts_cells, "substitution counts");
    L.units = j.alloc<u64>(units_cells, "dwell units");
    L.dropped_edges = j.alloc<u64>(edge_cells, "dropped edges");
    if (!d_edge || !d_slot || !d_rpow || !d_len || !d_off || !d_pois || !L.counts || !L.units || !L.dropped_edges) return false;
    // (pageable sources: the runtime stages them before it returns)
    if (!j.upload(d_edge, list.data(), edges, "upload history edges") ||
        !j.upload(d_slot, T->slot, R, "upload history tables") ||
        !j.upload(d_rpow, T->rpow, (size_t)T->nmat * T->kmax * S * S, "upload history tables") ||
        !j.upload(d_len, T->len, (size_t)edges * R, "upload history tables") ||
        !j.upload(d_off, T->off, (size_t)edges * R, "upload history tables") ||
        !j.upload(d_pois, T->pois, T->pois_count, "upload history tables") ||
        !hip_ok(hipMemsetAsync(L.counts, 0, (counts_cells ? counts_cells : 1) * sizeof(u64), j.stream), "hipMemsetAsync") ||
        !hip_ok(hipMemsetAsync(L.units, 0, (units_cells ? units_cells : 1) * sizeof(u64), j.stream), "hipMemsetAsync") ||
        !hip_ok(hipMemsetAsync(L.dropped_edges, 0, (edge_cells ? edge_cells : 1) * sizeof(u64), j.stream), "hipMemsetAsync"))
      return false;
    L.edges = edges;
    L.edge = d_edge;
    L.S = S; L.R = R; L.kmax = T->kmax;
    L.slot = d_slot; L.rpow = d_rpow; L.len = d_len; L.off = d_off; L.pois = d_pois;
    L.m = d_pattern_weights;
    L.seed = params->seed;
    return true;
  }

  bool launch(DeviceJob & j, const AncsStaged & s) override
  {
    if (!edges) return true;
    HistLaunch l = L;
    l.half = s.half;
    l.rows = s.rows; l.comp_row = s.comp_row;
    l.change_row = changes ? s.extra_row : HIST_NO;
    l.pitch = s.pitch;
    l.reps = s.reps; l.rep0 = s.rep0;
    l.first_replicate = params->first_replicate + s.rep0;
    l.site0 = s.col0; l.sites = s.cols;
    l.tiles = (s.cols + HIST_WG - 1) / HIST_WG;
    const u64 items = (u64)s.reps * edges * l.tiles;
    const unsigned grid = capped_grid("PLLHIP_HIST_BLOCKS", std::min<u64>(items, (u64)cu * 16));
    const size_t lds = ((size_t)l.S * l.S + (size_t)l.R * l.S) * sizeof(u64);
    // PLLHIP_HIST_LDS_BYTES=<n>: tables above n bytes are not kept in LDS (a test knob: at 1 every lane adds to memory
    // itself, the form partitions of more than 64 states would take)
    const char * knob = getenv("PLLHIP_HIST_LDS_BYTES");
    const size_t budget = knob && *knob ? std::min<size_t>(HIST_LDS_BYTES, strtoull(knob, nullptr, 10)) : HIST_LDS_BYTES;
    if (l.S <= HIST_LDS_STATES && lds <= budget)
      hipLaunchKernelGGL(k_history_edges<true>, dim3(grid), dim3(HIST_WG), lds, j.stream, l);
    else
      hipLaunchKernelGGL(k_history_edges<false>, dim3(grid), dim3(HIST_WG), 0, j.stream, l);
    return hip_ok(hipGetLastError(), "k_history_edges");
  }

  void deliver(const AncsStaged & s) override
  {
    if (!changes) return;
    for (unsigned r = 0; r < s.reps; ++r)
      for (unsigned e = 0; e < edges; ++e)
        memcpy(changes + ((size_t)(s.rep0 + r) * edges + e) * sites + s.col0,
               s.half + ((size_t)r * s.rows + s.extra_row + e) * s.pitch, s.cols);
  }

  bool finish(DeviceJob & j) override
  {
    return j.download(counts, L.counts, counts_cells, "download substitution counts") &&
           j.download(units, L.units, units_cells, "download dwell units") &&
           j.download(dropped_edges, L.dropped_edges, edge_cells, "download dropped edges") &&
           hip_ok(hipStreamSynchronize(j.stream), "download");
  }
};

int invalid(const char * who, const char * what)
{
  set_error(PLL_ERROR_PARAM_INVALID, "%s: %s", who, what);
  return PLL_FAILURE;
}

} // namespace

extern "C" {

PLL_EXPORT int pllhip_sample_histories_edges(pll_partition_t * partition, const pllhip_ancsample_params_t * params,
                                             unsigned int root_node, int root_scaler, unsigned int other_node,
                                             int other_scaler, unsigned int edge_count, const unsigned int * parent,
                                             const unsigned int * child, const unsigned int * matrix_indices,
                                             const unsigned int * freqs_indices, unsigned int node_count,
                                             const unsigned int * params_indices, const double * branch_lengths,
                                             unsigned char * out, unsigned char * component,
                                             unsigned long long * dropped, unsigned long long * counts,
                                             unsigned long long * units, unsigned char * changes,
                                             unsigned long long * dropped_edges)
{
  const char * who = "pllhip_sample_histories_edges";
  if (!partition || !partition->engine || !params || !freqs_indices || !params_indices || !counts || !units || !dropped_edges)
    return invalid(who, "the partition, the parameters, freqs_indices, params_indices or an output table is NULL");
  if (edge_count && (!parent || !child || !matrix_indices)) return invalid(who, "the edge list is NULL");
  if (edge_count && !branch_lengths) return invalid(who, "the branch lengths are NULL");
  if (params->flags & ~(unsigned)(PLLHIP_ANCS_TIPS | PLLHIP_ANCS_COMPONENT | PLLHIP_HIST_SITES))
    return invalid(who, "unknown flags");
  const bool with_sites = (params->flags & PLLHIP_HIST_SITES) != 0;
  if (with_sites && !changes) return invalid(who, "PLLHIP_HIST_SITES without a changes array");
  if (!engine_of(partition)->shards.empty()) return invalid(who, "sharded partitions are not supported");
  if (partition->states > 256 || partition->rate_cats > 128)
    return invalid(who, "more than 256 states or 128 categories do not fit the bytes of the draw");
  pllhip_history_tables_t * T = pllhip_history_tables_create(partition, edge_count, matrix_indices, params_indices,
                                                             branch_lengths, who);
  if (!T) return PLL_FAILURE;

  HistoryHook hook;
  hook.flags = PLLHIP_HIST_SITES;
  hook.extra_rows = with_sites ? edge_count : 0;
  const char * cap = getenv("PLLHIP_HIST_REPLICATES");
  hook.chunk_replicates = cap ? strtoull(cap, nullptr, 10) : 0;
  hook.partition = partition;
  hook.params = params;
  hook.T = T;
  hook.edges = edge_count;
  hook.sites = partition->sites;
  hook.parent = parent; hook.child = child; hook.matrix = matrix_indices;
  hook.counts = counts; hook.units = units; hook.dropped_edges = dropped_edges;
  hook.changes = with_sites ? changes : nullptr;
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  const int ok = ancsample_run(who, partition, params, root_node, root_scaler, other_node, other_scaler, edge_count,
                               parent, child, matrix_indices, freqs_indices, node_count, out, component, dropped, &hook, ms);
  pllhip_history_tables_destroy(T);
  if (ok && !partition->sites)                          // (no pattern, no launch: the tables are all zero)
  {
    const size_t cells = (size_t)params->replicates * edge_count;
    memset(counts, 0, cells * partition->states * partition->states * sizeof(u64));
    memset(units, 0, cells * partition->rate_cats * partition->states * sizeof(u64));
    memset(dropped_edges, 0, cells * sizeof(u64));
  }
  if (ok) memcpy(g_hist_ms, ms, sizeof(ms));
  return ok;
}

PLL_EXPORT void pllhip_history_last_times(double * table_ms, double * walk_ms, double * history_ms, double * copy_ms)
{
  if (table_ms) *table_ms = g_hist_ms[0];
  if (walk_ms) *walk_ms = g_hist_ms[1];
  if (history_ms) *history_ms = g_hist_ms[2];
  if (copy_ms) *copy_ms = g_hist_ms[3];
}

} // extern "C"
