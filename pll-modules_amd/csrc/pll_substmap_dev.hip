// pll_substmap_dev.hip -- the endpoint-pair table of an edge as a host result (pllhip_substmap_edge; contract:
// INTEGRATION.md, "Substitution mapping"; design: DESIGN.md section 31).
//
// One call: the scale pass, the pair kernel and the reduction on the partition's stream (substmap_scale / _pairs /
// _reduce, pll_core.hip: the kernel families live in that translation unit) with an event between them, one wait, one
// round of downloads.  Everything the call allocates on the device goes with its DeviceJob.
#include "device_job.hpp"
#include "pllhip.h"

#include <cstdlib>
#include <cstring>

using namespace pllhip;

namespace {

thread_local double g_last_ms[3] = {0.0, 0.0, 0.0};      // scale pass, pair kernel, reduction

} // namespace

extern "C" {

PLL_EXPORT void pllhip_edge_pairs_destroy(pllhip_edge_pairs_t * ep)
{
  if (!ep) return;
  free(ep->F); free(ep->pairs); free(ep->posterior); free(ep->differ);
  free(ep);
}

PLL_EXPORT pllhip_edge_pairs_t * pllhip_substmap_edge(pll_partition_t * partition, unsigned int parent_clv_index,
                                                      int parent_scaler_index, unsigned int child_clv_index,
                                                      int child_scaler_index, unsigned int matrix_index,
                                                      const unsigned int * freqs_indices, unsigned int flags)
{
  const char * who = "pllhip_substmap_edge";
  if (!partition || !partition->engine || !freqs_indices)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL partition or parameter indices", who);
    return nullptr;
  }
  if (flags & ~PLLHIP_SUBST_SITES)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: unknown flags", who);
    return nullptr;
  }
  Engine * e = engine_of(partition);
  if (!e->shards.empty())
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: sharded partitions are not supported", who);
    return nullptr;
  }
  const unsigned R = partition->rate_cats, N = e->Nreal, S = partition->states;
  for (unsigned r = 0; r < R; ++r)
    if (freqs_indices[r] >= partition->rate_matrices)
    {
      set_error(PLL_ERROR_PARAM_INVALID, "%s: parameter index %u of category %u is out of range", who, freqs_indices[r], r);
      return nullptr;
    }
  if (!check_category_weights(partition->rate_weights, R, who)) return nullptr;
  const bool sites = (flags & PLLHIP_SUBST_SITES) != 0;
  DeviceJob j;
  if (!j.enter(e->device, e->stream)) return nullptr;
  SubstmapShape shape;
  if (!substmap_shape(partition, freqs_indices, shape)) return nullptr;

  const size_t cells = (size_t)R * S * S, table = (size_t)R * shape.plane;
  pllhip_edge_pairs_t * ep = (pllhip_edge_pairs_t *)calloc(1, sizeof(*ep));
  if (ep)
  {
    ep->states = S; ep->cats = R; ep->sites = N;
    ep->F = (double *)calloc(cells, sizeof(double));
    ep->pairs = (double *)calloc(cells, sizeof(double));
    ep->posterior = (double *)calloc(R, sizeof(double));
    if (sites) ep->differ = (double *)calloc(N ? N : 1, sizeof(double));
  }
  if (!ep || !ep->F || !ep->pairs || !ep->posterior || (sites && !ep->differ))
  {
    pllhip_edge_pairs_destroy(ep);
    set_error(PLL_ERROR_MEM_ALLOC, "%s: cannot allocate the result", who);
    return nullptr;
  }
  for (unsigned n = 0; n < N; ++n) ep->weight_sum += (double)partition->pattern_weights[n];

  SubstmapBuffers buf;
  buf.A = j.alloc<double>(table, "site-category table");
  buf.B = shape.pinv ? j.alloc<double>(table, "site-category table") : nullptr;
  buf.A0 = sites ? j.alloc<double>(table, "site-category table") : nullptr;
  buf.c = j.alloc<unsigned>(N, "site-category counts");
  buf.m = j.alloc<unsigned>(N, "pattern weights");
  buf.scale = j.alloc<double>((size_t)R * shape.splane, "pair-table scale plane");
  buf.differ = sites ? j.alloc<double>(N, "per-site differences") : nullptr;
  buf.dropped = j.alloc<unsigned long long>(1, "dropped sites");
  buf.pm0 = sites ? j.alloc<double>(shape.pm_cells, "zeroed-diagonal matrices") : nullptr;
  buf.lut0 = (sites && shape.lut_cells) ? j.alloc<double>(shape.lut_cells, "zeroed-diagonal lookup tables") : nullptr;
  buf.partial = j.alloc<double>((size_t)shape.grid * cells, "partial pair tables");
  buf.F = j.alloc<double>(cells, "pair table");
  buf.pairs = j.alloc<double>(cells, "pair table");
  hipEvent_t t[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ok = buf.A && (!shape.pinv || buf.B) && (!sites || (buf.A0 && buf.differ && buf.pm0 && (!shape.lut_cells || buf.lut0))) &&
            buf.c && buf.m && buf.scale && buf.dropped && buf.partial && buf.F && buf.pairs &&
            // (pageable source: the copy has left the partition's array when the call returns, which waits below)
            j.upload(buf.m, partition->pattern_weights, N, "upload pattern weights") &&
            (t[0] = j.mark()) != nullptr &&
            substmap_scale(partition, parent_clv_index, parent_scaler_index, child_clv_index, child_scaler_index,
                           matrix_index, freqs_indices, shape, buf) &&
            (t[1] = j.mark()) != nullptr &&
            substmap_pairs(partition, parent_clv_index, child_clv_index, shape, buf) &&
            (t[2] = j.mark()) != nullptr &&
            substmap_reduce(partition, matrix_index, freqs_indices, shape, buf) &&
            (t[3] = j.mark()) != nullptr &&
            j.download(ep->F, buf.F, cells, "download") && j.download(ep->pairs, buf.pairs, cells, "download") &&
            j.download(&ep->dropped, buf.dropped, 1, "download") &&
            (!sites || !N || j.download(ep->differ, buf.differ, N, "download")) &&
            hip_ok(hipStreamSynchronize(e->stream), "pair table");
  if (!ok)
  {
    (void)hipStreamSynchronize(e->stream);           // (nothing may still write the buffers when they go)
    pllhip_edge_pairs_destroy(ep);
    return nullptr;
  }
  for (unsigned k = 0; k < 3; ++k)
  {
    float ms = 0.f;
    if (j.elapsed(t[k], t[k + 1], &ms)) g_last_ms[k] = ms;
  }
  for (unsigned r = 0; r < R; ++r)
  {
    double sum = 0.0;
    for (size_t x = 0; x < (size_t)S * S; ++x) sum += ep->pairs[(size_t)r * S * S + x];
    ep->posterior[r] = sum;
  }
  return ep;
}

PLL_EXPORT void pllhip_substmap_last_times(double * scale_ms, double * pairs_ms, double * reduce_ms)
{
  if (scale_ms) *scale_ms = g_last_ms[0];
  if (pairs_ms) *pairs_ms = g_last_ms[1];
  if (reduce_ms) *reduce_ms = g_last_ms[2];
}

} // extern "C"
