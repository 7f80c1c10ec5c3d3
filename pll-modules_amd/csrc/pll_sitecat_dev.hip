// pll_sitecat_dev.hip -- site-category sets: the per-site, per-category table of an edge kept on the device, the
// posteriors, site rates and expected counts read from it, and the EM fit of the category weights (contract:
// INTEGRATION.md, "Site categories"; design: DESIGN.md section 30).
//
// A set lives on one device with a stream of its own.  The table of an edge is written by the family's kernel on the
// partition's stream (sitecat_edge_table, pll_core.hip: the kernel families live in that translation unit) and waited
// for before pllhip_sitecat_edge returns, so a set does not depend on its partition afterwards.  The table is kept
// rate-major (planes of `plane` doubles); the [sites][cats] order of the interface is made at download.
#include "device_job.hpp"
#include "kernels_sitecat_sums.hpp"
#include "pllhip.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pllhip;

struct pllhip_sitecat
{
  int device = -1;
  hipStream_t stream = nullptr;
  unsigned N = 0, R = 0;
  size_t plane = 0;
  double * d_A = nullptr, * d_B = nullptr;    // [R][plane]; B null: no invariant part
  unsigned * d_c = nullptr;                   // [N]; null: all 0
  unsigned * d_m = nullptr;                   // [N] pattern weights; null: 1 each
  double * d_w = nullptr;                     // [R] the weights of the running call
  double * d_rho = nullptr;                   // [R]; null: a set without rates
  double * d_block = nullptr;                 // [SITECAT_RC + 1][SITECAT_MAX_GRID]
  unsigned * d_ticket = nullptr;
  double * h_sums = nullptr;                  // pinned, device-mapped: the results of one k_sitecat_expect
  double * d_sums = nullptr;                  // its device view
  std::vector<double> weights;                // the snapshot
  double msum = 0.0;                          // sum of the pattern weights
  bool from_partition = false, asc = false;
};

namespace {

constexpr unsigned SITECAT_MAX_CATS = 256;
constexpr unsigned SITECAT_MAX_GRID = 1024;

thread_local double g_last_ms[3] = {0.0, 0.0, 0.0};      // table, posteriors, EM

unsigned sums_grid(unsigned N)
{
  return capped_grid("PLLHIP_SITECAT_BLOCKS", std::min<unsigned long long>(((unsigned long long)N + 255) / 256, SITECAT_MAX_GRID));
}

bool check_set(const pllhip_sitecat_t * set, const char * who)
{
  if (set) return true;
  set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL set", who);
  return false;
}

bool check_weights(const double * w, unsigned R, const char * who) { return check_category_weights(w, R, who); }

void release(pllhip_sitecat_t * set)
{
  if (!set) return;
  DeviceScope scope;
  if (set->device >= 0 && scope.enter(set->device))
  {
    if (set->stream) (void)hipStreamSynchronize(set->stream);
    for (void * p : {(void *)set->d_A, (void *)set->d_B, (void *)set->d_c, (void *)set->d_m, (void *)set->d_w,
                     (void *)set->d_rho, (void *)set->d_block, (void *)set->d_ticket})
      if (p) (void)hipFree(p);
    if (set->h_sums) (void)hipHostFree(set->h_sums);
    if (set->stream) (void)hipStreamDestroy(set->stream);
  }
  delete set;
}

// the buffers every set has; the device is current
bool allocate(pllhip_sitecat_t * set, bool with_B, bool with_c, bool with_m, bool with_rho)
{
  const size_t cells = (size_t)set->R * set->plane;
  if (!hip_ok(hipStreamCreateWithFlags(&set->stream, hipStreamNonBlocking), "hipStreamCreate")) return false;
  if (!dev_alloc(&set->d_A, cells, "site-category table") || (with_B && !dev_alloc(&set->d_B, cells, "site-category table")) ||
      (with_c && !dev_alloc(&set->d_c, set->N, "site-category counts")) ||
      (with_m && !dev_alloc(&set->d_m, set->N, "pattern weights")) || !dev_alloc(&set->d_w, set->R, "category weights") ||
      (with_rho && !dev_alloc(&set->d_rho, set->R, "category rates")) ||
      !dev_alloc(&set->d_block, (size_t)(SITECAT_RC + 1) * SITECAT_MAX_GRID, "block sums") ||
      !dev_alloc(&set->d_ticket, 1, "ticket") ||
      !hip_ok(hipHostMalloc(reinterpret_cast<void **>(&set->h_sums), sizeof(double) * (SITECAT_RC + 1), hipHostMallocMapped),
              "hipHostMalloc sums"))
    return false;
  return hip_ok(hipHostGetDevicePointer(reinterpret_cast<void **>(&set->d_sums), set->h_sums, 0), "hipHostGetDevicePointer") &&
         hip_ok(hipMemsetAsync(set->d_ticket, 0, sizeof(unsigned), set->stream), "memset ticket");
}

SiteCatTable table_of(const pllhip_sitecat_t * set)
{
  SiteCatTable t;
  t.A = set->d_A; t.B = set->d_B; t.c = set->d_c; t.plane = set->plane; t.N = set->N; t.R = set->R;
  return t;
}

// expected[R] and sum_n m_n lnl[n] at the weights in d_w: one launch and one wait per SITECAT_RC rates
bool expect(pllhip_sitecat_t * set, double * expected, double * loglh)
{
  const unsigned grid = sums_grid(set->N);
  for (unsigned r0 = 0; r0 < set->R; r0 += SITECAT_RC)
  {
    hipLaunchKernelGGL(k_sitecat_expect, dim3(grid), dim3(256), 0, set->stream, table_of(set), set->d_w, set->d_m, r0,
                       set->d_block, set->d_ticket, set->d_sums);
    if (!hip_ok(hipGetLastError(), "expectation kernel") || !hip_ok(hipStreamSynchronize(set->stream), "expectation kernel"))
      return false;
    for (unsigned k = 0; k < SITECAT_RC && r0 + k < set->R; ++k) expected[r0 + k] = set->h_sums[k];
    *loglh = set->h_sums[SITECAT_RC];
  }
  return true;
}

bool upload_weights_of_call(pllhip_sitecat_t * set, const double * w)
{
  // (pageable source: the copy has left `w` when the call returns)
  return hip_ok(hipMemcpyAsync(set->d_w, w, sizeof(double) * set->R, hipMemcpyHostToDevice, set->stream), "upload weights") &&
         hip_ok(hipStreamSynchronize(set->stream), "upload weights");
}

// rate-major planes -> out[n][r]
void to_site_major(const std::vector<double> & planes, size_t plane, unsigned N, unsigned R, double * out)
{
  for (unsigned r = 0; r < R; ++r)
    for (unsigned n = 0; n < N; ++n) out[(size_t)n * R + r] = planes[(size_t)r * plane + n];
}

double now_ms()
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

} // namespace

extern "C" {

PLL_EXPORT pllhip_sitecat_t * pllhip_sitecat_edge(pll_partition_t * partition, unsigned int parent_clv_index,
                                                  int parent_scaler_index, unsigned int child_clv_index,
                                                  int child_scaler_index, unsigned int matrix_index,
                                                  const unsigned int * freqs_indices)
{
  const char * who = "pllhip_sitecat_edge";
  if (!partition || !partition->engine || !freqs_indices)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL partition or parameter indices", who);
    return nullptr;
  }
  Engine * e = engine_of(partition);
  if (!e->shards.empty())
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: sharded partitions are not supported", who);
    return nullptr;
  }
  const unsigned R = partition->rate_cats, N = e->Nreal;
  bool pinv = false;
  for (unsigned r = 0; r < R; ++r)
  {
    if (freqs_indices[r] >= partition->rate_matrices)
    {
      set_error(PLL_ERROR_PARAM_INVALID, "%s: parameter index %u of category %u is out of range", who, freqs_indices[r], r);
      return nullptr;
    }
    pinv = pinv || partition->prop_invar[freqs_indices[r]] > 0.0;
  }
  if (!check_weights(partition->rate_weights, R, who)) return nullptr;
  DeviceScope scope;
  if (!scope.enter(e->device)) return nullptr;
  pllhip_sitecat_t * set = new pllhip_sitecat;
  set->device = e->device;
  set->N = N;
  set->R = R;
  set->plane = ((size_t)N + 1) & ~(size_t)1;
  set->from_partition = true;
  set->asc = (partition->attributes & PLL_ATTRIB_AB_MASK) != 0;
  set->weights.assign(partition->rate_weights, partition->rate_weights + R);
  for (unsigned n = 0; n < N; ++n) set->msum += (double)partition->pattern_weights[n];
  hipEvent_t t0 = nullptr, t1 = nullptr;
  bool ok = allocate(set, pinv, true, true, true) &&
            hip_ok(hipMemcpyAsync(set->d_m, partition->pattern_weights, sizeof(unsigned) * N, hipMemcpyHostToDevice, set->stream), "upload pattern weights") &&
            hip_ok(hipMemcpyAsync(set->d_rho, partition->rates, sizeof(double) * R, hipMemcpyHostToDevice, set->stream), "upload rates") &&
            hip_ok(hipStreamSynchronize(set->stream), "upload") &&
            hip_ok(hipEventCreate(&t0), "hipEventCreate") && hip_ok(hipEventCreate(&t1), "hipEventCreate");
  if (ok)
  {
    SiteCatPlanes planes;
    planes.A = set->d_A; planes.B = set->d_B; planes.c = set->d_c; planes.plane = set->plane;
    ok = hip_ok(hipEventRecord(t0, e->stream), "hipEventRecord") &&
         sitecat_edge_table(partition, parent_clv_index, parent_scaler_index, child_clv_index, child_scaler_index,
                            matrix_index, freqs_indices, planes) &&
         hip_ok(hipEventRecord(t1, e->stream), "hipEventRecord") && hip_ok(hipStreamSynchronize(e->stream), "table kernel");
    float ms = 0.f;
    if (ok && hipEventElapsedTime(&ms, t0, t1) == hipSuccess) g_last_ms[0] = ms;
  }
  if (t0) (void)hipEventDestroy(t0);
  if (t1) (void)hipEventDestroy(t1);
  if (ok) return set;
  (void)hipStreamSynchronize(e->stream);         // (nothing may still write the planes when they go)
  release(set);
  return nullptr;
}

PLL_EXPORT pllhip_sitecat_t * pllhip_sitecat_from_table(unsigned int sites, unsigned int cats, const double * g,
                                                        const unsigned int * pattern_weights, const double * weights)
{
  const char * who = "pllhip_sitecat_from_table";
  if (!g || !sites || !cats || cats > SITECAT_MAX_CATS)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: no table, or not 1 .. %u categories", who, SITECAT_MAX_CATS);
    return nullptr;
  }
  for (size_t x = 0; x < (size_t)sites * cats; ++x)
    if (!(g[x] >= 0.0) || !std::isfinite(g[x]))
    {
      set_error(PLL_ERROR_PARAM_INVALID, "%s: the entry of site %zu, category %zu is negative or not finite", who,
                x / cats, x % cats);
      return nullptr;
    }
  std::vector<double> w(cats, 1.0 / cats);
  if (weights) w.assign(weights, weights + cats);
  if (!check_weights(w.data(), cats, who)) return nullptr;
  int device = 0;
  DeviceScope scope;
  if (!caller_device(who, &device) || !scope.enter(device)) return nullptr;
  pllhip_sitecat_t * set = new pllhip_sitecat;
  set->device = device;
  set->N = sites;
  set->R = cats;
  set->plane = ((size_t)sites + 1) & ~(size_t)1;
  set->weights = w;
  if (pattern_weights) for (unsigned n = 0; n < sites; ++n) set->msum += (double)pattern_weights[n];
  else set->msum = (double)sites;
  std::vector<double> planes((size_t)cats * set->plane, 0.0);
  for (unsigned n = 0; n < sites; ++n)
    for (unsigned r = 0; r < cats; ++r) planes[(size_t)r * set->plane + n] = g[(size_t)n * cats + r];
  const bool ok = allocate(set, false, false, pattern_weights != nullptr, false) &&
                  hip_ok(hipMemcpyAsync(set->d_A, planes.data(), sizeof(double) * planes.size(), hipMemcpyHostToDevice, set->stream), "upload table") &&
                  (!pattern_weights || hip_ok(hipMemcpyAsync(set->d_m, pattern_weights, sizeof(unsigned) * sites, hipMemcpyHostToDevice, set->stream), "upload pattern weights")) &&
                  hip_ok(hipStreamSynchronize(set->stream), "upload table");
  if (ok) return set;
  release(set);
  return nullptr;
}

PLL_EXPORT void pllhip_sitecat_destroy(pllhip_sitecat_t * set) { release(set); }
PLL_EXPORT unsigned int pllhip_sitecat_sites(const pllhip_sitecat_t * set) { return set ? set->N : 0; }
PLL_EXPORT unsigned int pllhip_sitecat_categories(const pllhip_sitecat_t * set) { return set ? set->R : 0; }

PLL_EXPORT int pllhip_sitecat_table(pllhip_sitecat_t * set, double * rate_part, double * inv_part, unsigned int * counts)
{
  if (!check_set(set, "pllhip_sitecat_table")) return PLL_FAILURE;
  DeviceScope scope;
  if (!scope.enter(set->device)) return PLL_FAILURE;
  const size_t cells = (size_t)set->R * set->plane;
  std::vector<double> planes(cells);
  if (rate_part)
  {
    PLLHIP_TRY(hipMemcpyAsync(planes.data(), set->d_A, sizeof(double) * cells, hipMemcpyDeviceToHost, set->stream));
    PLLHIP_TRY(hipStreamSynchronize(set->stream));
    to_site_major(planes, set->plane, set->N, set->R, rate_part);
  }
  if (inv_part)
  {
    if (set->d_B)
    {
      PLLHIP_TRY(hipMemcpyAsync(planes.data(), set->d_B, sizeof(double) * cells, hipMemcpyDeviceToHost, set->stream));
      PLLHIP_TRY(hipStreamSynchronize(set->stream));
      to_site_major(planes, set->plane, set->N, set->R, inv_part);
    }
    else memset(inv_part, 0, sizeof(double) * set->N * set->R);
  }
  if (counts)
  {
    if (set->d_c)
    {
      PLLHIP_TRY(hipMemcpyAsync(counts, set->d_c, sizeof(unsigned) * set->N, hipMemcpyDeviceToHost, set->stream));
      PLLHIP_TRY(hipStreamSynchronize(set->stream));
    }
    else memset(counts, 0, sizeof(unsigned) * set->N);
  }
  return PLL_SUCCESS;
}

PLL_EXPORT void pllhip_site_posteriors_destroy(pllhip_site_posteriors_t * po)
{
  if (!po) return;
  free(po->rate); free(po->category); free(po->category_prob); free(po->invariant_prob); free(po->lnl);
  free(po->posterior); free(po->expected);
  free(po);
}

PLL_EXPORT pllhip_site_posteriors_t * pllhip_sitecat_posteriors(pllhip_sitecat_t * set, const double * weights,
                                                                unsigned int flags)
{
  const char * who = "pllhip_sitecat_posteriors";
  if (!check_set(set, who)) return nullptr;
  if (flags & ~PLLHIP_SITECAT_POSTERIORS)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: unknown flags", who);
    return nullptr;
  }
  const double * w = weights ? weights : set->weights.data();
  if (!check_weights(w, set->R, who)) return nullptr;
  const unsigned N = set->N, R = set->R;
  const bool full = (flags & PLLHIP_SITECAT_POSTERIORS) != 0, rates = set->d_rho != nullptr;
  DeviceJob j;
  if (!j.enter(set->device, set->stream)) return nullptr;
  pllhip_site_posteriors_t * po = (pllhip_site_posteriors_t *)calloc(1, sizeof(*po));
  if (po)
  {
    po->sites = N;
    po->cats = R;
    if (rates) po->rate = (double *)calloc(N, sizeof(double));
    if (rates) po->invariant_prob = (double *)calloc(N, sizeof(double));
    po->category = (unsigned char *)calloc(N, 1);
    po->category_prob = (double *)calloc(N, sizeof(double));
    po->lnl = (double *)calloc(N, sizeof(double));
    if (full) po->posterior = (double *)calloc((size_t)N * R, sizeof(double));
    po->expected = (double *)calloc(R, sizeof(double));
  }
  if (!po || (rates && (!po->rate || !po->invariant_prob)) || !po->category || !po->category_prob || !po->lnl ||
      (full && !po->posterior) || !po->expected)
  {
    pllhip_site_posteriors_destroy(po);
    set_error(PLL_ERROR_MEM_ALLOC, "%s: cannot allocate the results", who);
    return nullptr;
  }
  SiteCatPost out;
  out.rate = rates ? j.alloc<double>(N, "site rates") : nullptr;
  out.inv = rates ? j.alloc<double>(N, "invariant posteriors") : nullptr;
  out.category = j.alloc<uint8_t>(N, "site categories");
  out.category_prob = j.alloc<double>(N, "category posteriors");
  out.lnl = j.alloc<double>(N, "per-site lnL");
  out.post = full ? j.alloc<double>((size_t)R * set->plane, "posterior table") : nullptr;
  std::vector<double> planes(full ? (size_t)R * set->plane : 0);
  hipEvent_t t0 = nullptr, t1 = nullptr;
  bool ok = (!rates || (out.rate && out.inv)) && out.category && out.category_prob && out.lnl && (!full || out.post) &&
            upload_weights_of_call(set, w) && (t0 = j.mark()) != nullptr;
  if (ok)
  {
    hipLaunchKernelGGL(k_sitecat_posterior, dim3(sums_grid(N)), dim3(256), 0, set->stream, table_of(set), set->d_w,
                       set->d_rho, out);
    ok = hip_ok(hipGetLastError(), "posterior kernel") && expect(set, po->expected, &po->loglh) && (t1 = j.mark()) != nullptr &&
         (!rates || (j.download(po->rate, out.rate, N, "download") && j.download(po->invariant_prob, out.inv, N, "download"))) &&
         j.download(po->category, out.category, N, "download") && j.download(po->category_prob, out.category_prob, N, "download") &&
         j.download(po->lnl, out.lnl, N, "download") &&
         (!full || j.download(planes.data(), out.post, planes.size(), "download")) &&
         hip_ok(hipStreamSynchronize(set->stream), "download");
    float ms = 0.f;
    if (ok && j.elapsed(t0, t1, &ms)) g_last_ms[1] = ms;
  }
  if (!ok)
  {
    pllhip_site_posteriors_destroy(po);
    return nullptr;
  }
  if (full) to_site_major(planes, set->plane, N, R, po->posterior);
  return po;
}

PLL_EXPORT int pllhip_sitecat_em_weights(pllhip_sitecat_t * set, const pllhip_sitecat_em_params_t * params,
                                         double * weights, double * loglh, unsigned int * iterations,
                                         double * trail_weights, double * trail_loglh)
{
  const char * who = "pllhip_sitecat_em_weights";
  if (!check_set(set, who)) return PLL_FAILURE;
  if (!params || !weights)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL parameters or weights", who);
    return PLL_FAILURE;
  }
  if (set->asc)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: the partition has an ascertainment-bias correction, which depends on the weights", who);
    return PLL_FAILURE;
  }
  if (!(params->epsilon >= 0.0))
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: epsilon is negative or not a number", who);
    return PLL_FAILURE;
  }
  const unsigned R = set->R;
  std::vector<double> w(params->start ? params->start : set->weights.data(), (params->start ? params->start : set->weights.data()) + R);
  if (!check_weights(w.data(), R, who)) return PLL_FAILURE;
  if (!(set->msum > 0.0))
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: the pattern weights add up to 0", who);
    return PLL_FAILURE;
  }
  DeviceScope scope;
  if (!scope.enter(set->device)) return PLL_FAILURE;
  const double t_begin = now_ms();
  std::vector<double> expected(R);
  double L = 0.0, Lprev = 0.0;
  unsigned i = 0;
  for (;; ++i)
  {
    if (!upload_weights_of_call(set, w.data()) || !expect(set, expected.data(), &L)) return PLL_FAILURE;
    if (i < PLLHIP_SITECAT_TRAIL_MAX)
    {
      if (trail_weights) memcpy(trail_weights + (size_t)i * R, w.data(), sizeof(double) * R);
      if (trail_loglh) trail_loglh[i] = L;
    }
    if (!(L > -INFINITY))
    {
      // rare: name the site (the first with a pattern weight and no likelihood under these weights)
      std::vector<double> A((size_t)R * set->N), B;
      std::vector<unsigned> m(set->N, 1u);
      if (set->d_B) B.resize(A.size());
      if (!pllhip_sitecat_table(set, A.data(), set->d_B ? B.data() : nullptr, nullptr)) return PLL_FAILURE;
      if (set->d_m && !hip_ok(hipMemcpy(m.data(), set->d_m, sizeof(unsigned) * set->N, hipMemcpyDeviceToHost), "download")) return PLL_FAILURE;
      unsigned bad = set->N;
      for (unsigned n = 0; n < set->N && bad == set->N; ++n)
      {
        double T = 0.0;
        for (unsigned r = 0; r < R; ++r) T += w[r] * (A[(size_t)n * R + r] + (set->d_B ? B[(size_t)n * R + r] : 0.0));
        if (m[n] && !(T > 0.0)) bad = n;
      }
      set_error(PLL_ERROR_PARAM_INVALID, "%s: site %u has a pattern weight and likelihood 0 under the weights of iteration %u", who, bad, i);
      return PLL_FAILURE;
    }
    if ((i > 0 && L - Lprev < params->epsilon) || i == params->max_iterations) break;
    // (sum_r expected[r] is sum_n m_n up to rounding; as the divisor it makes the new weights add up to 1 to R roundings)
    double esum = 0.0;
    for (unsigned r = 0; r < R; ++r) esum += expected[r];
    for (unsigned r = 0; r < R; ++r) w[r] = expected[r] / esum;
    Lprev = L;
  }
  memcpy(weights, w.data(), sizeof(double) * R);
  if (loglh) *loglh = L;
  if (iterations) *iterations = i;
  g_last_ms[2] = now_ms() - t_begin;
  return PLL_SUCCESS;
}

PLL_EXPORT void pllhip_sitecat_last_times(double * table_ms, double * posterior_ms, double * em_ms)
{
  if (table_ms) *table_ms = g_last_ms[0];
  if (posterior_ms) *posterior_ms = g_last_ms[1];
  if (em_ms) *em_ms = g_last_ms[2];
}

} // extern "C"
