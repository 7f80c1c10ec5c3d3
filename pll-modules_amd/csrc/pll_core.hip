// pll_core.hip -- the hot path of include/pll.h (tier B0) on gfx950, plus the
// engine services behind it and the pllhip_* extension API.
//
// Entry points and the reference call sites they serve:
//   pll_update_prob_matrices           src/tree/treeinfo.c:854 (count = 1 per branch!)
//   pll_update_partials                src/tree/treeinfo.c:1037,
//                                      src/optimize/pll_optimize.c:748-775 (count = 1)
//   pll_compute_edge_loglikelihood     src/tree/treeinfo.c:1049
//   pll_compute_root_loglikelihood     src/optimize/pll_optimize.c:329
//   pll_update_sumtable                src/optimize/pll_optimize.c:800, 1468
//   pll_compute_likelihood_derivatives src/optimize/pll_optimize.c:307, 1151, 1249
//
// Execution model: one HIP stream per partition; every call enqueues kernels
// and returns, except the calls that return a scalar (lnL, derivatives), which
// copy <= 16 KB of per-block partial sums to pinned host memory, synchronise
// and finish the sum on the host in a fixed order (bit-reproducible).
// Operation lists are level-scheduled: ops of one dependency level share one
// launch (grid.y = op), their descriptors travel by value in the kernel
// arguments, so no host->device copy sits on the critical path.
#include "chain_plan.hpp"
#include "device_job.hpp"
#include "kernels_common.hpp"
#include "kernels_generic.hpp"
#include "kernels_s4.hpp"
#include "kernels_s20.hpp"
#include "kernels_s61.hpp"
#include "kernels_s16.hpp"
#include "kernels_repeats.hpp"
#include "kernels_newton_s4.hpp"
#include "kernels_ancestral.hpp"
#include "kernels_sitecat.hpp"
#include "kernels_substmap.hpp"
#include "kernels_ancsample.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <time.h>

namespace pllhip {

using namespace chainplan;                       // the chain planner (chain_plan.hpp)

static thread_local int g_device = -1;

bool hip_ok(hipError_t e, const char * what)
{
  if (e == hipSuccess) return true;
  set_error(PLL_ERROR_HIP_RUNTIME, "HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
  return false;
}

static int current_device()
{
  if (g_device < 0)
  {
    const char * env = getenv("PLLHIP_DEVICE");
    g_device = env ? atoi(env) : 0;
  }
  return g_device;
}

int flush_pmatrices(pll_partition_t * p);
static int ensure_luts(pll_partition_t * p);
static int update_partials_impl(pll_partition_t * p, const pll_operation_t * ops, unsigned count);

// Store the vectors of `want` that exist as their operation only (Engine::ledger): the operations that made them run
// again as an ordinary list -- the same kernels on the same inputs, so what is stored is what the traversal would have
// stored.  A member of a deferred run brings the members above it along, one launch for the run instead of one per
// member (UnstoredLedger::recompute_list; PLLHIP_DEFER_GROUP=0: every reader stores what it reads and what lies below)
static int store_unstored(Engine * e, const std::vector<unsigned> & want, const std::vector<char> * going = nullptr)
{
  if (e->ledger.empty()) return PLL_SUCCESS;
  static const int env_group = getenv("PLLHIP_DEFER_GROUP") ? atoi(getenv("PLLHIP_DEFER_GROUP")) : 1;
  std::vector<pll_operation_t> list;
  unsigned ndeferred = 0;
  e->ledger.recompute_list(want, env_group != 0, going, list, ndeferred);
  if (list.empty()) return PLL_SUCCESS;
  const bool mode = e->transient_mode;
  e->transient_busy = true;
  e->transient_mode = false;
  const int rc = update_partials_impl(e->owner, list.data(), (unsigned)list.size());
  e->transient_mode = mode;
  e->transient_busy = false;
  if (rc) e->ledger.stored((unsigned)list.size() - ndeferred, ndeferred);
  return rc;
}

static int transient_flush_all(Engine * e)
{
  if (e->ledger.empty() || e->transient_busy) return PLL_SUCCESS;
  std::vector<unsigned> all;
  for (unsigned n = 0; n < e->nodes; ++n) if (e->ledger.live(n)) all.push_back(n);
  return store_unstored(e, all);
}

static bool cherry_storage(Engine * e, unsigned node, unsigned nclasses);
// tip lookup tables exist: PLL_ATTRIB_PATTERN_TIP, or the engine's own codes (Engine::shadow_codes)
static bool lut_active(const Engine * e) { return e->coded_tips || e->shadow_codes; }
static unsigned codes_in_use(const Engine * e, const pll_partition_t * p)
{
  return e->shadow_codes ? (unsigned)e->shadow_tipmap.size() : p->maxstates;
}
// the operations above tip `idx` read it through byte codes and lookup tables
static bool tip_coded(const Engine * e, unsigned idx)
{
  return idx < e->tips && (e->coded_tips || (e->shadow_codes && e->tip_has_codes[idx]));
}
static void batch_free(BatchPlan * b);
static void batch_free_hook(BatchPlan * b) { batch_free(b); }

// ---------------------------------------------------------------------------
// engine-internal sharding: which devices the partitions created next are spread over
// ---------------------------------------------------------------------------
static thread_local std::vector<int> g_shard_devices;
static thread_local bool g_shard_devices_set = false;
static thread_local bool g_building_shards = false;

static std::vector<int> shard_devices()
{
  if (!g_shard_devices_set)
  {
    g_shard_devices_set = true;
    if (const char * env = getenv("PLLHIP_SHARD_DEVICES"))
      for (const char * c = env; *c; )
      {
        char * end = nullptr;
        const long v = strtol(c, &end, 10);
        if (end == c) break;
        g_shard_devices.push_back((int)v);
        c = (*end == ',') ? end + 1 : end;
      }
  }
  return g_shard_devices;
}

static ModelView model_view(const Engine * e)
{
  ModelView mv;
  mv.base = e->d_model;
  mv.off_rates = (unsigned)e->off_rates;
  mv.off_weights = (unsigned)e->off_weights;
  mv.off_pinv = (unsigned)e->off_pinv;
  mv.off_freqs = (unsigned)e->off_freqs;
  mv.off_evals = (unsigned)e->off_evals;
  mv.off_evecs = (unsigned)e->off_evecs;
  mv.off_ievecs = (unsigned)e->off_ievecs;
  mv.S = e->S;
  mv.Sp = e->Sp;
  return mv;
}

// Kernel arguments in device memory (the ROCm runtime's HIP_FORCE_DEV_KERNARG): by default they sit in
// host memory, and the first wave of every workgroup pays a trip over the fabric for its operation
// descriptors -- 3 to 5 us on a kernel that runs for 10 (an SPR insertion's partial traversal, a
// 25 k-site codon slice: W3 -3 ... -6 %, C5 at 25 k sites 1.73 -> 1.65 ms per step).  Set when the
// library is loaded, i.e. before its first HIP call, unless the user has decided otherwise; a runtime
// that another component initialised earlier keeps its setting.
// The setting is process-global and setenv() is not safe against a concurrent getenv() in another thread of a
// host application that dlopen()s this library late: such an application sets HIP_FORCE_DEV_KERNARG itself
// before it starts threads (what bench.py and the tools do) and switches this off -- at run time with
// PLLHIP_SET_RUNTIME_DEFAULTS=0, or at build time with -DPLLHIP_NO_RUNTIME_DEFAULTS.
#ifndef PLLHIP_NO_RUNTIME_DEFAULTS
__attribute__((constructor)) static void pllhip_runtime_defaults()
{
  const char * opt = getenv("PLLHIP_SET_RUNTIME_DEFAULTS");
  if (opt && !atoi(opt)) return;
  if (!getenv("HIP_FORCE_DEV_KERNARG")) setenv("HIP_FORCE_DEV_KERNARG", "1", 0);
  // GPU_MAX_HW_QUEUES is left alone.  The runtime multiplexes a process's streams onto that many hardware queues (four
  // by default), in order within a queue; sixteen would give every partition stream its own -- which the Newton-Raphson
  // loop over several partitions needs (newton_multi_enabled) -- but cost the many-stream workloads a third of their
  // rate on one box: 64 DNA partitions of 10 k sites 3.6 -> 5.7 ms per evaluation, 32 protein partitions 5.6 -> 6.9,
  // 16 x 60 k DNA 3.3 -> 4.0 (tools/gpu_r4_queues.sh; between the two, 6 / 8 / 12 queues cost the same).
}
#endif

// partitions alive per device (whole-traversal launches are the default for a partition that has
// its device to itself)
static std::atomic<int> engines_on_device[64];

Engine * engine_create(pll_partition_t * p)
{
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
  {
    set_error(PLL_ERROR_HIP_NODEVICE,
              "No HIP device available: the likelihood engine has no CPU fallback");
    return nullptr;
  }
  const int dev = current_device();
  if (dev >= ndev)
  {
    set_error(PLL_ERROR_HIP_NODEVICE, "HIP device %d requested, %d visible", dev, ndev);
    return nullptr;
  }
  // spread over several devices?  (not for the shards themselves, tiny partitions, or AB partitions:
  // their correction needs the constant patterns and the total pattern weight in one place)
  const std::vector<int> devs = g_building_shards ? std::vector<int>() : shard_devices();
  if (devs.size() >= 2 && !p->asc_bias_alloc && p->sites >= 64u * devs.size())
  {
    Engine * r = new (std::nothrow) Engine();
    if (!r) { set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate engine state"); return nullptr; }
    r->device = dev;
    r->S = p->states; r->Sp = p->states_padded; r->R = p->rate_cats; r->N = r->Nreal = p->sites;
    r->tips = p->tips; r->nodes = p->nodes; r->nscalers = p->scale_buffers;
    r->nmat = p->prob_matrices; r->nrm = p->rate_matrices;
    r->coded_tips = (p->attributes & PLL_ATTRIB_PATTERN_TIP) != 0;
    r->rate_scalers = (p->attributes & PLL_ATTRIB_RATE_SCALERS) != 0;
    const unsigned K = (unsigned)devs.size();
    const unsigned chunk = ((p->sites + K - 1) / K + S20_BS - 1) / S20_BS * S20_BS;   // whole 32-site blocks
    const int saved = g_device;
    g_building_shards = true;
    bool ok = true;
    for (unsigned k = 0; ok && k < K; ++k)
    {
      const unsigned first = std::min(p->sites, k * chunk), last = std::min(p->sites, (k + 1) * chunk);
      if (first == last) break;
      if (devs[k] < 0 || devs[k] % ndev != devs[k]) { /* wrap: lets a test shard over one visible device */ }
      g_device = ((devs[k] % ndev) + ndev) % ndev;
      pll_partition_t * c = pll_partition_create(p->tips, p->clv_buffers, p->states, last - first, p->rate_matrices,
                                                 p->prob_matrices, p->rate_cats, p->scale_buffers,
                                                 p->attributes & ~PLLHIP_ATTRIB_HOST_MIRRORS);
      ok = c != nullptr;
      if (ok) { r->shards.push_back(c); r->shard_first.push_back(first); }
    }
    g_building_shards = false;
    g_device = saved;
    if (!ok || r->shards.size() < 2)
    {
      for (pll_partition_t * c : r->shards) pll_partition_destroy(c);
      delete r;
      if (!ok) return nullptr;
    }
    else
    {
      r->shard_first.push_back(p->sites);
      r->family = engine_of(r->shards[0])->family;
      p->engine = r;
      return r;
    }
  }
  if (!hip_ok(hipSetDevice(dev), "hipSetDevice")) return nullptr;

  Engine * e = new (std::nothrow) Engine();
  if (!e)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate engine state");
    return nullptr;
  }
  e->device = dev;
  e->S = p->states; e->Sp = p->states_padded; e->R = p->rate_cats;
  e->Nreal = p->sites;
  e->N = p->sites + (p->asc_bias_alloc ? (unsigned)p->asc_additional_sites : 0u);
  e->tips = p->tips; e->nodes = p->nodes; e->nscalers = p->scale_buffers;
  e->nmat = p->prob_matrices; e->nrm = p->rate_matrices;
  e->coded_tips = (p->attributes & PLL_ATTRIB_PATTERN_TIP) != 0;
  e->tip_has_codes.assign(p->tips, 0);
  e->rate_scalers = (p->attributes & PLL_ATTRIB_RATE_SCALERS) != 0;
  // PLLHIP_SITE_REPEATS=0: never; =2: as if every partition had the attribute (the whole test suite under site repeats)
  const int env_repeats = getenv("PLLHIP_SITE_REPEATS") ? atoi(getenv("PLLHIP_SITE_REPEATS")) : 1;
  // (without PLL_ATTRIB_PATTERN_TIP -- libpll's own combination: the two attributes exclude one another there -- the
  // tips given through pll_set_tip_states are class nodes from the start: upload_tip_classes)
  // (ascertainment-bias columns are sites like any other for the class maps: weight 0, a class of their own each)
  e->site_repeats = ((p->attributes & PLL_ATTRIB_SITE_REPEATS) != 0 || env_repeats == 2) && !e->rate_scalers &&
                    env_repeats != 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess) e->cu_count = prop.multiProcessorCount;

  const char * force = getenv("PLLHIP_FORCE_GENERIC");
  static const int no_s16 = getenv("PLLHIP_NO_S16") ? atoi(getenv("PLLHIP_NO_S16")) : 0;
  if (force && atoi(force)) e->family = KernelFamily::Generic;
  // per-rate scalers: every matrix-core family carries them (4 states go to the 2..16-state
  // family: the VALU 4-state kernels vote per site)
  else if (e->rate_scalers && e->S <= 16) e->family = no_s16 ? KernelFamily::Generic : KernelFamily::S16;
  else if (e->S == 4 && (e->R & (e->R - 1)) == 0) e->family = KernelFamily::S4;
  else if (e->S == 20 && e->R <= 8) e->family = KernelFamily::S20;
  // 33 .. 64 states: the codon family (61 states: its own instantiation with the state count at compile time)
  else if (e->S >= 33 && e->S <= 64) e->family = KernelFamily::S61;
  // 2 .. 32 states (17 .. 32: two M tiles): every alphabet the 4- and 20-state families do not take
  else if (s16_supported(e->S, e->R) && !no_s16) e->family = KernelFamily::S16;
  else e->family = KernelFamily::Generic;
  e->blocked = (e->family == KernelFamily::S20 || e->family == KernelFamily::S61 || e->family == KernelFamily::S16);
  // (PLLHIP_TIP_CLASSES=0: tips of partitions without pattern tips as vectors only)
  e->shadow_codes = e->family == KernelFamily::S61 && !e->coded_tips && p->asc_bias_alloc == 0 &&
                    !(getenv("PLLHIP_TIP_CLASSES") && atoi(getenv("PLLHIP_TIP_CLASSES")) == 0);
  e->rows = !e->blocked ? 0u : (e->family == KernelFamily::S16) ? 4u * ((e->S + 3u) / 4u)
                               : (e->family == KernelFamily::S61) ? S61_SP : e->Sp;
  e->nblk = (e->N + S20_BS - 1) / S20_BS;
  e->Nalloc = e->blocked ? e->nblk * S20_BS : e->N;
  e->sc_len = (size_t)e->Nalloc * (e->rate_scalers ? e->R : 1);

  bool ok = hip_ok(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking), "hipStreamCreate");
  if (ok) { e->counted = true; ++engines_on_device[e->device & 63]; }
  const size_t clv_len = e->blocked ? (size_t)e->nblk * e->R * e->rows * S20_BS : (size_t)e->N * e->R * e->Sp;
  e->clv_len = clv_len;
  e->d_clv.assign(e->nodes, nullptr);
  e->d_codes.assign(e->tips, nullptr);
  for (unsigned i = 0; ok && i < e->nodes; ++i)
  {
    // (33 .. 64 states without pattern tips: codes of the engine's own next to the vector)
    if (i < e->tips && e->shadow_codes)
      ok = dev_alloc(&e->d_codes[i], (size_t)e->Nalloc, "tip codes") &&
           hip_ok(hipMemsetAsync(e->d_codes[i], 0, e->Nalloc ? e->Nalloc : 1, e->stream), "memset codes");
    if (i < e->tips && e->coded_tips)
      ok = dev_alloc(&e->d_codes[i], (size_t)e->Nalloc, "tip codes") &&
           hip_ok(hipMemsetAsync(e->d_codes[i], 0, e->Nalloc ? e->Nalloc : 1, e->stream), "memset codes");
    else
      ok = dev_alloc(&e->d_clv[i], clv_len, "CLV") &&
           hip_ok(hipMemsetAsync(e->d_clv[i], 0, (clv_len ? clv_len : 1) * sizeof(double), e->stream),
                  "memset CLV");
  }
  const size_t pm_len = (size_t)e->nmat * e->R * e->S * e->Sp;
  ok = ok && dev_alloc(&e->d_scalers, (size_t)e->nscalers * e->sc_len, "scalers");
  ok = ok && hip_ok(hipMemsetAsync(e->d_scalers, 0,
                                   std::max<size_t>(1, (size_t)e->nscalers * e->sc_len) * sizeof(unsigned),
                                   e->stream), "memset scalers");
  ok = ok && dev_alloc(&e->d_pmat, pm_len, "P-matrices");
  if (e->family == KernelFamily::S20)
    ok = ok && dev_alloc(&e->d_pfrag, std::max<size_t>(1, (size_t)e->nmat * e->R * 400), "P-matrix fragments") &&
         hip_ok(hipMemsetAsync(e->d_pfrag, 0, std::max<size_t>(1, (size_t)e->nmat * e->R * 400) * sizeof(double), e->stream),
                "memset fragments");
  ok = ok && hip_ok(hipMemsetAsync(e->d_pmat, 0, std::max<size_t>(1, pm_len) * sizeof(double), e->stream),
                    "memset pmat");
  ok = ok && dev_alloc(&e->d_weights, (size_t)e->N, "pattern weights");
  ok = ok && dev_alloc(&e->d_tipmap, (size_t)PLL_ASCII_SIZE, "tipmap");
  ok = ok && hip_ok(hipMemsetAsync(e->d_tipmap, 0, PLL_ASCII_SIZE * sizeof(unsigned long long), e->stream),
                    "memset tipmap");
  ok = ok && dev_alloc(&e->d_partials, (size_t)REDUCE_QUANTITIES * REDUCE_BLOCKS, "reduction partials");
  ok = ok && dev_alloc(&e->d_counter, (size_t)REDUCE_COUNTER_WORDS, "reduction tickets");
  ok = ok && hip_ok(hipMemsetAsync(e->d_counter, 0, REDUCE_COUNTER_WORDS * sizeof(unsigned), e->stream),
                    "memset tickets");
  ok = ok && hip_ok(hipHostMalloc(reinterpret_cast<void **>(&e->h_result), RESULT_WORDS * sizeof(double),
                                  hipHostMallocMapped), "hipHostMalloc result");
  if (ok) memset(e->h_result, 0, RESULT_WORDS * sizeof(double));   // the sequence word starts at 0 (recycled pinned pages)
  ok = ok && hip_ok(hipHostGetDevicePointer(reinterpret_cast<void **>(&e->d_result), e->h_result, 0),
                    "hipHostGetDevicePointer");
  if (const char * ff = getenv("PLLHIP_FUSED_FINISH")) e->fused_finish = atoi(ff) != 0;
  if (p->asc_bias_alloc)
  {
    const size_t bytes = sizeof(double) * MAX_TRIAL_LENGTHS * 64 * 4;
    ok = ok && hip_ok(hipHostMalloc(reinterpret_cast<void **>(&e->h_asc), bytes, hipHostMallocMapped), "hipHostMalloc asc");
    if (ok) memset(e->h_asc, 0, bytes);
    ok = ok && hip_ok(hipHostGetDevicePointer(reinterpret_cast<void **>(&e->d_asc), e->h_asc, 0), "map asc");
  }
  // (the 2 .. 32-state family: where it runs operation chains -- four rate categories, per-site scaling)
  const bool class_family = e->family == KernelFamily::S20 || e->family == KernelFamily::S4 ||
                            (e->family == KernelFamily::S16 && chains_supported_s16(e));
  // Tips that are vectors (no PLL_ATTRIB_PATTERN_TIP) but came through pll_set_tip_states are known per class of sites
  // -- the state masks -- whether or not the partition asks for site repeats: the operations above them read them as
  // wide tips (4 bytes per site and a row table per branch instead of R * S * 8 bytes per site; bit for bit the same
  // values: upload_tip_classes).  PLLHIP_TIP_CLASSES=0: tips as vectors only.
  static const int env_tip_classes = getenv("PLLHIP_TIP_CLASSES") ? atoi(getenv("PLLHIP_TIP_CLASSES")) : 1;
  e->tip_classes = env_tip_classes != 0 && !e->coded_tips && !e->rate_scalers && class_family;
  if ((e->site_repeats || e->tip_classes) && class_family)
  {
    e->cherries.assign(e->nodes, Engine::Cherry());
    e->tip_version.assign(e->tips, 0);
    e->scaler_lazy.assign(e->nscalers, -1);
  }
  if (!class_family) e->site_repeats = false;   // (the 61-state family, other rate counts of the 2 .. 32-state one: not yet)
  e->pmat_brlen.assign(e->nmat, std::numeric_limits<double>::quiet_NaN());
  e->pmat_params.assign(e->nmat, std::vector<unsigned>());
  e->owner = p;
  e->ledger.reset(e->nodes, e->nmat);
  e->transient_mode = getenv("PLLHIP_TRANSIENT") && atoi(getenv("PLLHIP_TRANSIENT")) != 0;

  // model block layout
  size_t off = 0;
  e->off_rates = off;   off += e->R;
  e->off_weights = off; off += e->R;
  e->off_pinv = off;    off += e->nrm;
  e->off_freqs = off;   off += (size_t)e->nrm * e->Sp;
  e->off_evals = off;   off += (size_t)e->nrm * e->Sp;
  e->off_evecs = off;   off += (size_t)e->nrm * e->S * e->Sp;
  e->off_ievecs = off;  off += (size_t)e->nrm * e->S * e->Sp;
  e->model_len = off;
  ok = ok && dev_alloc(&e->d_model, e->model_len, "model block");
  e->model_shadow.assign(e->model_len, std::numeric_limits<double>::quiet_NaN());

  if (!ok)
  {
    engine_destroy(e);
    return nullptr;
  }
  p->engine = e;
  if (!upload_weights(p))
  {
    p->engine = nullptr;
    engine_destroy(e);
    return nullptr;
  }
  return e;
}

void engine_destroy(Engine * e)
{
  if (!e) return;
  if (!e->shards.empty())
  {
    for (pll_partition_t * c : e->shards) pll_partition_destroy(c);
    delete e;
    return;
  }
  (void)hipSetDevice(e->device);
  if (e->counted) --engines_on_device[e->device & 63];
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (double * ptr : e->d_clv) if (ptr) (void)hipFree(ptr);
  for (uint8_t * ptr : e->d_codes) if (ptr) (void)hipFree(ptr);
  for (auto & kv : e->sumtables) (void)hipFree(kv.second);
  (void)hipFree(e->d_scalers);
  (void)hipFree(e->d_pmat);
  (void)hipFree(e->d_pfrag);
  (void)hipFree(e->d_lut);
  (void)hipFree(e->d_s61_votes);
  (void)hipFree(e->d_s61_ttscale);
  for (auto & slot : e->s61_pred) { if (slot.buf[0]) (void)hipFree(slot.buf[0]); if (slot.buf[1]) (void)hipFree(slot.buf[1]); }
  (void)hipFree(e->d_weights);
  (void)hipFree(e->d_invariant);
  (void)hipFree(e->d_tipmap);
  (void)hipFree(e->d_model);
  (void)hipFree(e->d_partials);
  (void)hipFree(e->d_persite);
  for (auto & c : e->cherries) { (void)hipFree(c.table); (void)hipFree(c.pair); (void)hipFree(c.flags); (void)hipFree(c.rep); (void)hipFree(c.counts); }
  (void)hipFree(e->d_class_seen);
  if (e->h_class_total) (void)hipHostFree(e->h_class_total);
  (void)hipFree(e->d_pairlut);
  (void)hipFree(e->d_looktab);
  (void)hipFree(e->d_newton);
  if (e->newton_ready) (void)hipEventDestroy(e->newton_ready);
  if (e->newton_done) (void)hipEventDestroy(e->newton_done);
  if (e->h_newton) (void)hipHostFree(e->h_newton);
  (void)hipFree(e->d_sum_scratch);
  if (e->h_result) (void)hipHostFree(e->h_result);
  if (e->h_asc) (void)hipHostFree(e->h_asc);
  (void)hipFree(e->d_counter);
  batch_free_hook(e->batch);
  (void)hipFree(e->plan.d_buf);
  if (e->plan.h_stage) (void)hipHostFree(e->plan.h_stage);
  if (e->plan.copied) (void)hipEventDestroy(e->plan.copied);
  for (auto & ev : e->prof_events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

// the small model arrays of a sharded partition live in the parent (the caller writes them
// there); every routed call that depends on them copies them to the shards first
static void push_model(const pll_partition_t * p, pll_partition_t * c)
{
  const size_t S = p->states, Sp = p->states_padded;
  memcpy(c->rates, p->rates, sizeof(double) * p->rate_cats);
  memcpy(c->rate_weights, p->rate_weights, sizeof(double) * p->rate_cats);
  memcpy(c->prop_invar, p->prop_invar, sizeof(double) * p->rate_matrices);
  memcpy(c->eigen_decomp_valid, p->eigen_decomp_valid, sizeof(int) * p->rate_matrices);
  for (unsigned m = 0; m < p->rate_matrices; ++m)
  {
    memcpy(c->frequencies[m], p->frequencies[m], sizeof(double) * Sp);
    memcpy(c->subst_params[m], p->subst_params[m], sizeof(double) * S * (S - 1) / 2);
    // an eigen-system that differs from the shard's copy (the parent decomposed again, or a caller wrote
    // the arrays): the shard's next model check has to look at it, also inside a burst of P-matrix requests
    if (memcmp(c->eigenvals[m], p->eigenvals[m], sizeof(double) * Sp) != 0 ||
        memcmp(c->eigenvecs[m], p->eigenvecs[m], sizeof(double) * S * Sp) != 0 ||
        memcmp(c->inv_eigenvecs[m], p->inv_eigenvecs[m], sizeof(double) * S * Sp) != 0)
    {
      memcpy(c->eigenvals[m], p->eigenvals[m], sizeof(double) * Sp);
      memcpy(c->eigenvecs[m], p->eigenvecs[m], sizeof(double) * S * Sp);
      memcpy(c->inv_eigenvecs[m], p->inv_eigenvecs[m], sizeof(double) * S * Sp);
      engine_of(c)->eigen_touched = true;
    }
  }
}

int upload_weights(pll_partition_t * p)
{
  Engine * e = engine_of(p);
  if (!e) return PLL_SUCCESS;   // called from the constructor before the engine exists
  if (!e->shards.empty())
  {
    for (size_t k = 0; k < e->shards.size(); ++k)
      pll_set_pattern_weights(e->shards[k], p->pattern_weights + e->shard_first[k]);
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  // the ascertainment-bias columns weigh nothing in the sums over the alignment: their part of
  // the likelihood is the correction the host applies (the host array keeps their state weights)
  e->weights_shadow.assign(p->pattern_weights, p->pattern_weights + e->N);
  for (unsigned n = e->Nreal; n < e->N; ++n) e->weights_shadow[n] = 0;
  if (e->N)
  {
    PLLHIP_TRY(hipMemcpyAsync(e->d_weights, e->weights_shadow.data(), (size_t)e->N * sizeof(unsigned),
                              hipMemcpyHostToDevice, e->stream));
    PLLHIP_TRY(hipStreamSynchronize(e->stream));      // the source is this engine's own buffer: keep it simple
  }
  return PLL_SUCCESS;
}

int upload_tipmap(pll_partition_t * p)
{
  Engine * e = engine_of(p);
  if (!lut_active(e) || e->tipmap_codes_uploaded == codes_in_use(e, p)) return PLL_SUCCESS;
  if (e->shadow_codes)
  {
    std::vector<unsigned long long> tm(PLL_ASCII_SIZE, 0ULL);
    std::copy(e->shadow_tipmap.begin(), e->shadow_tipmap.end(), tm.begin());
    PLLHIP_TRY(hipMemcpyAsync(e->d_tipmap, tm.data(), PLL_ASCII_SIZE * sizeof(unsigned long long), hipMemcpyHostToDevice, e->stream));
    PLLHIP_TRY(hipStreamSynchronize(e->stream));               // (a local source)
  }
  else
    PLLHIP_TRY(hipMemcpyAsync(e->d_tipmap, p->tipmap, PLL_ASCII_SIZE * sizeof(unsigned long long),
                              hipMemcpyHostToDevice, e->stream));
  e->tipmap_codes_uploaded = codes_in_use(e, p);
  return PLL_SUCCESS;
}

int upload_tip_codes(pll_partition_t * p, unsigned tip)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    // the shards take the parent's codes and code table as they are (a checkpoint loader wrote them)
    for (size_t k = 0; k < e->shards.size(); ++k)
    {
      pll_partition_t * c = e->shards[k];
      memcpy(c->tipchars[tip], p->tipchars[tip] + e->shard_first[k], c->sites);
      memcpy(c->tipmap, p->tipmap, sizeof(pll_state_t) * PLL_ASCII_SIZE);
      memcpy(c->charmap, p->charmap, PLL_ASCII_SIZE);
      if (c->maxstates != p->maxstates) { c->maxstates = p->maxstates; invalidate_luts(c); }
      engine_of(c)->tipmap_codes_uploaded = ~0u;
      if (!upload_tip_codes(c, tip)) return PLL_FAILURE;
    }
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  if (!transient_flush_all(e)) return PLL_FAILURE;           // vectors that exist as their operation only read the old codes
  if (e->N)
    PLLHIP_TRY(hipMemcpyAsync(e->d_codes[tip], p->tipchars[tip], (size_t)e->N,
                              hipMemcpyHostToDevice, e->stream));
  if (tip < e->tip_version.size()) e->tip_version[tip] = ++e->class_clock;     // class maps above this tip are stale
  return upload_tipmap(p);
}

// device staging buffer that frees itself on every exit path
struct DevTmp
{
  double * ptr = nullptr;
  ~DevTmp() { if (ptr) (void)hipFree(ptr); }
};

// API layout [site][rate][Sp] on the host -> device layout of the family
static int store_clv(Engine * e, double * d_dst, const double * host_clv)
{
  const size_t len = (size_t)e->N * e->R * e->Sp;
  if (!len) return PLL_SUCCESS;
  if (!e->blocked)
  {
    PLLHIP_TRY(hipMemcpyAsync(d_dst, host_clv, len * sizeof(double), hipMemcpyHostToDevice, e->stream));
    PLLHIP_TRY(hipStreamSynchronize(e->stream));
    return PLL_SUCCESS;
  }
  DevTmp tmp;
  if (!dev_alloc(&tmp.ptr, len, "layout staging")) return PLL_FAILURE;
  PLLHIP_TRY(hipMemcpyAsync(tmp.ptr, host_clv, len * sizeof(double), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_s20_to_blocked, dim3(e->cu_count * 8), dim3(256), 0, e->stream,
                     tmp.ptr, d_dst, e->N, e->nblk, e->R, e->Sp, e->rows);
  PLLHIP_TRY(hipGetLastError());
  PLLHIP_TRY(hipStreamSynchronize(e->stream));
  return PLL_SUCCESS;
}

// device layout of the family -> API layout on the host
static int fetch_clv(Engine * e, const double * d_src, double * host_out)
{
  const size_t len = (size_t)e->N * e->R * e->Sp;
  if (!len) return PLL_SUCCESS;
  if (!e->blocked)
  {
    PLLHIP_TRY(hipMemcpyAsync(host_out, d_src, len * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    PLLHIP_TRY(hipStreamSynchronize(e->stream));
    return PLL_SUCCESS;
  }
  DevTmp tmp;
  if (!dev_alloc(&tmp.ptr, len, "layout staging")) return PLL_FAILURE;
  hipLaunchKernelGGL(k_s20_from_blocked, dim3(e->cu_count * 8), dim3(256), 0, e->stream,
                     d_src, tmp.ptr, e->N, e->R, e->Sp, e->rows);
  PLLHIP_TRY(hipGetLastError());
  PLLHIP_TRY(hipMemcpyAsync(host_out, tmp.ptr, len * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  PLLHIP_TRY(hipStreamSynchronize(e->stream));
  return PLL_SUCCESS;
}

int upload_tip_clv(pll_partition_t * p, unsigned tip, const double * host_clv)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    for (size_t k = 0; k < e->shards.size(); ++k)
      if (!upload_tip_clv(e->shards[k], tip, host_clv + (size_t)e->shard_first[k] * e->R * e->Sp)) return PLL_FAILURE;
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  if (!transient_flush_all(e)) return PLL_FAILURE;
  if (e->shadow_codes) e->tip_has_codes[tip] = 0;               // (pll_set_tip_states brings the codes afterwards)
  if (!e->cherries.empty())
  {
    // whatever classes the tip had are not those of the new vector (pll_set_tip_states tells them afterwards)
    e->cherries[tip].valid = false;
    e->tip_version[tip] = ++e->class_clock;
    e->plan.key.clear();
  }
  return store_clv(e, e->d_clv[tip], host_clv);
}

// Site repeats without PLL_ATTRIB_PATTERN_TIP (the combination libpll itself allows; the reference's harness:
// test/src/common.c:15-31, "tv" and "sr" are separate switches): a tip set through pll_set_tip_states is a vector
// AND a class node -- the class of a site is its state mask, the table the masks' 0/1 vectors -- so that the
// operations above it are computed per class exactly as above coded tips: class maps from its classes, its rows
// through the P-matrix of its branch with the MFMA sequence of an inner child (bit for bit what the vector gives).
// site_class[n] < nclasses, masks[class] = the state set.
int upload_tip_classes(pll_partition_t * p, unsigned tip, const unsigned * site_class, const unsigned long long * masks,
                       unsigned nclasses)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    for (size_t k = 0; k < e->shards.size(); ++k)
      if (!upload_tip_classes(e->shards[k], tip, site_class + e->shard_first[k], masks, nclasses)) return PLL_FAILURE;
    return PLL_SUCCESS;
  }
  if (e->shadow_codes && nclasses && e->N)
  {
    // 33 .. 64 states: the tip's classes become codes of the engine's own table (the state masks met so far, all tips)
    PLLHIP_TRY(hipSetDevice(e->device));
    std::vector<unsigned> code_of(nclasses, 0u);
    const size_t before = e->shadow_tipmap.size();
    for (unsigned k = 0; k < nclasses; ++k)
    {
      size_t c = 0;
      for (; c < e->shadow_tipmap.size(); ++c) if (e->shadow_tipmap[c] == masks[k]) break;
      if (c == e->shadow_tipmap.size())
      {
        if (c >= 255) { e->shadow_tipmap.resize(before); return PLL_SUCCESS; }    // (too many codes: the tip stays a vector)
        e->shadow_tipmap.push_back(masks[k]);
      }
      code_of[k] = (unsigned)c;
    }
    std::vector<uint8_t> codes(e->Nalloc, 0);
    for (unsigned n = 0; n < e->N; ++n) codes[n] = (uint8_t)code_of[site_class[n] < nclasses ? site_class[n] : 0u];
    PLLHIP_TRY(hipMemcpyAsync(e->d_codes[tip], codes.data(), codes.size(), hipMemcpyHostToDevice, e->stream));
    PLLHIP_TRY(hipStreamSynchronize(e->stream));
    e->tip_has_codes[tip] = 1;
    if (e->shadow_tipmap.size() != before) { e->lut_stale = true; e->plan.key.clear(); }
    return upload_tipmap(p);
  }
  if (e->coded_tips || e->cherries.empty() || !nclasses || !e->N) return PLL_SUCCESS;
  PLLHIP_TRY(hipSetDevice(e->device));
  Engine::Cherry & c = e->cherries[tip];
  if (!cherry_storage(e, tip, nclasses)) return PLL_FAILURE;
  if (!c.pair && !dev_alloc(&c.pair, (size_t)e->Nalloc, "class codes")) return PLL_FAILURE;
  std::vector<unsigned> cls(e->Nalloc, 0u);                       // (padding sites: class 0)
  for (unsigned n = 0; n < e->N; ++n) cls[n] = site_class[n] < nclasses ? site_class[n] : 0u;
  PLLHIP_TRY(hipMemcpyAsync(c.pair, cls.data(), cls.size() * sizeof(unsigned), hipMemcpyHostToDevice, e->stream));
  // the table: a pseudo alignment of the classes in the API layout, brought into the layout of the family's tables
  const unsigned npblk = (nclasses + S20_BS - 1) / S20_BS;
  std::vector<double> api((size_t)nclasses * e->R * e->Sp, 0.0);
  for (unsigned k = 0; k < nclasses; ++k)
    for (unsigned r = 0; r < e->R; ++r)
      for (unsigned j = 0; j < e->S; ++j)
        api[((size_t)k * e->R + r) * e->Sp + j] = (double)((masks[k] >> j) & 1ULL);
  DevTmp tmp;
  if (e->blocked)
  {
    if (!dev_alloc(&tmp.ptr, api.size(), "class table staging")) return PLL_FAILURE;
    PLLHIP_TRY(hipMemcpyAsync(tmp.ptr, api.data(), api.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_s20_to_blocked, dim3(std::max(1u, std::min(npblk * e->R, e->cu_count * 8u))), dim3(256), 0, e->stream,
                       tmp.ptr, c.table, nclasses, npblk, e->R, e->Sp, e->rows);
    PLLHIP_TRY(hipGetLastError());
  }
  else
    PLLHIP_TRY(hipMemcpyAsync(c.table, api.data(), api.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  PLLHIP_TRY(hipStreamSynchronize(e->stream));                    // (the sources are local)
  (void)hipFree(c.rep); c.rep = nullptr; c.rep_cap = 0;
  c.nclasses = nclasses;
  c.ncodes = 0;
  c.valid = c.materialized = c.map_valid = c.trackable = true;
  c.scaler_index = PLL_SCALE_BUFFER_NONE;
  c.child[0] = c.child[1] = ~0u;
  c.version = e->tip_version[tip] = ++e->class_clock;
  e->plan.key.clear();
  return PLL_SUCCESS;
}

void invalidate_luts(pll_partition_t * p)
{
  Engine * e = engine_of(p);
  if (e) e->lut_stale = true;
  if (e) for (pll_partition_t * c : e->shards) invalidate_luts(c);
}

// host model arrays -> device if anything changed since the last call.  The arrays are compared
// in place against the shadow of what the device holds (no copy, no allocation: the reference
// issues one pll_update_prob_matrices call per branch, 397 per C3 evaluation).
// light: only the arrays a caller pokes between two consecutive P-matrix requests (rates, weights,
// p-inv, frequencies); the eigen-systems -- 2 S Sp doubles per rate matrix, 63 KiB at 61 states --
// were compared by the first request of the burst and change only through ensure_eigen, which
// runs before this.
int sync_model(pll_partition_t * p, bool light)
{
  Engine * e = engine_of(p);
  const double * sh = e->model_shadow.data();
  bool same = e->model_shadow.size() == e->model_len &&
              memcmp(sh + e->off_rates, p->rates, sizeof(double) * e->R) == 0 &&
              memcmp(sh + e->off_weights, p->rate_weights, sizeof(double) * e->R) == 0 &&
              memcmp(sh + e->off_pinv, p->prop_invar, sizeof(double) * e->nrm) == 0;
  for (unsigned m = 0; same && m < e->nrm; ++m)
  {
    same = memcmp(sh + e->off_freqs + (size_t)m * e->Sp, p->frequencies[m], sizeof(double) * e->Sp) == 0;
    if (same && !(light && !e->eigen_touched))
      same = memcmp(sh + e->off_evals + (size_t)m * e->Sp, p->eigenvals[m], sizeof(double) * e->Sp) == 0 &&
             memcmp(sh + e->off_evecs + (size_t)m * e->S * e->Sp, p->inv_eigenvecs[m], sizeof(double) * e->S * e->Sp) == 0 &&
             memcmp(sh + e->off_ievecs + (size_t)m * e->S * e->Sp, p->eigenvecs[m], sizeof(double) * e->S * e->Sp) == 0;
  }
  if (!light) e->pmatrix_burst = false;
  e->eigen_touched = false;
  if (same) return PLL_SUCCESS;

  std::vector<double> cur(e->model_len, 0.0);
  memcpy(&cur[e->off_rates], p->rates, sizeof(double) * e->R);
  memcpy(&cur[e->off_weights], p->rate_weights, sizeof(double) * e->R);
  memcpy(&cur[e->off_pinv], p->prop_invar, sizeof(double) * e->nrm);
  for (unsigned m = 0; m < e->nrm; ++m)
  {
    memcpy(&cur[e->off_freqs + (size_t)m * e->Sp], p->frequencies[m], sizeof(double) * e->Sp);
    memcpy(&cur[e->off_evals + (size_t)m * e->Sp], p->eigenvals[m], sizeof(double) * e->Sp);
    // device slots: evecs = V, ievecs = V^-1; the partition fields follow libpll-2's naming,
    // where `inv_eigenvecs` is V and `eigenvecs` is V^-1 (pll_model.cpp)
    memcpy(&cur[e->off_evecs + (size_t)m * e->S * e->Sp], p->inv_eigenvecs[m], sizeof(double) * e->S * e->Sp);
    memcpy(&cur[e->off_ievecs + (size_t)m * e->S * e->Sp], p->eigenvecs[m], sizeof(double) * e->S * e->Sp);
  }
  // queued P-matrix requests belong to the model state they were issued under,
  // which is the one still on the device
  if (!flush_pmatrices(p)) return PLL_FAILURE;
  PLLHIP_TRY(hipSetDevice(e->device));
  // pageable source: the runtime stages it before returning, so `cur` may die
  PLLHIP_TRY(hipMemcpyAsync(e->d_model, cur.data(), sizeof(double) * e->model_len,
                            hipMemcpyHostToDevice, e->stream));
  PLLHIP_TRY(hipStreamSynchronize(e->stream));
  e->model_shadow.swap(cur);
  e->counters.model_uploads++;
  e->model_generation++;
  // pattern weights (4*N bytes) are NOT re-compared here: pll-modules changes them
  // only through pll_set_pattern_weights (SURVEY.md section 0.3 lists the fields it
  // pokes directly; weights are not among them), which uploads them itself.
  return PLL_SUCCESS;
}

// Launch the queued P-matrix requests.  pll-modules asks for one matrix per call
// (src/tree/treeinfo.c:845-865: 2n-3 calls per evaluation); the requests are
// queued on the host and go to the device up to 200 per launch as soon as a
// consumer of P-matrices (partials, lnL, host mirror) or a model change needs them.
int flush_pmatrices(pll_partition_t * p)
{
  Engine * e = engine_of(p);
  if (e->pend_midx.empty()) return PLL_SUCCESS;
  PLLHIP_TRY(hipSetDevice(e->device));
  // a vector that an evaluate-only traversal did not store is recomputed with the matrices it was made with: stored
  // now, before one of them changes (an operation list gives the vectors it overwrites up BEFORE it comes here)
  if (!e->ledger.empty() && !e->transient_busy)
    for (unsigned m : e->pend_midx)
      if (e->ledger.matrix_in_use(m))
      {
        if (!transient_flush_all(e)) return PLL_FAILURE;
        break;
      }
  if (lut_active(e))
  {
    // LUT storage must exist so that the kernel can fill it in the same pass
    const bool stale = e->lut_stale || !e->d_lut || e->lut_codes < std::max(1u, codes_in_use(e, p));
    if (stale && !ensure_luts(p)) return PLL_FAILURE;
  }
  const ModelView mv = model_view(e);
  // operands staged in LDS when two S x Sp matrices fit the kernel's register tiling (S <= 64)
  const int staged = (size_t)e->S * e->Sp <= 4096;
  const size_t lds = staged ? sizeof(double) * 2 * (size_t)(e->Sp == 64 ? 64 : e->S) * e->Sp   // 64 columns: whole 64 x 64 operands (matrix cores)
                            : sizeof(double) * ((size_t)e->Sp + (size_t)e->S * e->Sp);
  const unsigned count = (unsigned)e->pend_midx.size();
  for (unsigned base = 0; base < count; base += MAX_PMAT_PER_LAUNCH)
  {
    const unsigned nb = std::min(MAX_PMAT_PER_LAUNCH, count - base);
    PmatBatch batch;
    for (unsigned q = 0; q < nb; ++q)
    {
      batch.midx[q] = e->pend_midx[base + q];
      batch.t[q] = e->pend_t[base + q];
      e->pend_pos[batch.midx[q]] = -1;
    }
    hipLaunchKernelGGL(k_pmatrix, dim3(nb, e->R), dim3(256), lds, e->stream,
                       mv, e->pend_params, batch, e->R, e->d_pmat,
                       lut_active(e) ? e->d_lut : nullptr, e->lut_codes, e->d_tipmap, staged, e->d_pfrag);
    PLLHIP_TRY(hipGetLastError());
    e->counters.pmatrix_launches++;
  }
  e->pend_midx.clear();
  e->pend_t.clear();
  e->pmat_host_dirty = true;
  return PLL_SUCCESS;
}

static int ensure_eigen(pll_partition_t * p, const unsigned * params_indices)
{
  for (unsigned r = 0; r < p->rate_cats; ++r)
  {
    const unsigned idx = params_indices[r];
    if (idx >= p->rate_matrices)
    {
      set_error(PLL_ERROR_PARAM_INVALID, "params index %u out of range", idx);
      return PLL_FAILURE;
    }
    if (!p->eigen_decomp_valid[idx])
    {
      if (!update_eigen_host(p, idx)) return PLL_FAILURE;
      engine_of(p)->eigen_touched = true;           // the next model check looks at the eigen-systems as well
    }
  }
  return PLL_SUCCESS;
}

static ParamIdx make_params(const pll_partition_t * p, const unsigned * idx)
{
  ParamIdx pi;
  memset(&pi, 0, sizeof(pi));
  for (unsigned r = 0; r < p->rate_cats; ++r) pi.v[r] = idx[r];
  return pi;
}

// LUT storage exists once tips are coded; (re)build when the code table grew
static int ensure_luts(pll_partition_t * p)
{
  Engine * e = engine_of(p);
  if (!lut_active(e)) return PLL_SUCCESS;
  if (!upload_tipmap(p)) return PLL_FAILURE;
  const unsigned want = std::max(1u, codes_in_use(e, p));
  if (!e->d_lut || e->lut_codes < want)
  {
    // grow with head-room so that a few late codes do not re-allocate
    // (but never past the size the 20-/61-state kernels can stage in LDS: 30 / 67 codes)
    unsigned cap = std::min<unsigned>(PLL_ASCII_SIZE, std::max(want, (e->S == 4) ? 16u : want + 8u));
    if (e->family == KernelFamily::S61 && want <= S61_FRAGS / e->S) cap = std::min(cap, S61_FRAGS / e->S);   // 67 at 61 states
    if (e->family == KernelFamily::S20 && want <= 30u) cap = std::min(cap, 30u);
    // (2 .. 32 states: ... nor past what the family stages in LDS, S16_LUT_LDS doubles per table, while the codes in use fit)
    if (e->family == KernelFamily::S16 && e->R * want * e->S <= S16_LUT_LDS) cap = std::min(cap, std::max(want, S16_LUT_LDS / (e->R * e->S)));
    if (e->d_lut) { PLLHIP_TRY(hipStreamSynchronize(e->stream)); (void)hipFree(e->d_lut); e->d_lut = nullptr; }
    e->plan.key.clear();                            // cached schedules point into the old tables
    if (!dev_alloc(&e->d_lut, (size_t)e->nmat * e->R * cap * e->S, "tip lookup tables")) return PLL_FAILURE;
    e->lut_codes = cap;
    e->lut_stale = true;
  }
  if (e->lut_stale && e->nmat)
  {
    hipLaunchKernelGGL(k_rebuild_lut, dim3(e->nmat, e->R), dim3(256), 0, e->stream,
                       e->S, e->Sp, e->R, e->d_pmat, e->d_lut, e->lut_codes, e->d_tipmap);
    PLLHIP_TRY(hipGetLastError());
  }
  e->lut_stale = false;
  return PLL_SUCCESS;
}

static int ensure_invariant(pll_partition_t * p)
{
  Engine * e = engine_of(p);
  bool need = false;
  for (unsigned m = 0; m < e->nrm; ++m) if (p->prop_invar[m] > 0.0) need = true;
  if (!need || !p->invariant) return PLL_SUCCESS;
  if (!e->d_invariant)
    if (!dev_alloc(&e->d_invariant, (size_t)e->N, "invariant sites")) return PLL_FAILURE;
  if (!e->invariant_uploaded)
  {
    PLLHIP_TRY(hipMemcpyAsync(e->d_invariant, p->invariant, (size_t)e->N * sizeof(int),
                              hipMemcpyHostToDevice, e->stream));
    e->invariant_uploaded = true;
  }
  return PLL_SUCCESS;
}

static NodeRef node_ref(const Engine * e, unsigned clv_index)
{
  NodeRef n;
  n.clv = e->d_clv[clv_index];
  // (the engine's own codes of a tip without PLL_ATTRIB_PATTERN_TIP serve the operations above it only: a reader of the
  // tip itself takes the vector)
  n.codes = (e->coded_tips && clv_index < e->tips) ? e->d_codes[clv_index] : nullptr;
  return n;
}

static const unsigned * scaler_ptr(const Engine * e, int idx)
{
  return (idx == PLL_SCALE_BUFFER_NONE) ? nullptr : e->d_scalers + (size_t)idx * e->sc_len;
}

// --- ascertainment-bias correction on the host (same formulas as oracle/orc_kernels.c) ---------
// from the log-likelihoods l[k] of the S constant patterns:
//   Lewis  - W log(1 - sum_k L_k);  Felsenstein  + w log(sum_k L_k);  Stamatakis  + sum_k w_k log(L_k)
static double asc_correction(const pll_partition_t * p, const double * l)
{
  const unsigned S = p->states;
  const unsigned * w = p->pattern_weights + p->sites;
  unsigned wsum = 0;
  double mx = l[0], sum = 0.0, corr = 0.0;
  for (unsigned k = 0; k < S; ++k) { mx = std::max(mx, l[k]); wsum += w[k]; }
  for (unsigned k = 0; k < S; ++k) sum += exp(l[k] - mx);
  switch (p->attributes & PLL_ATTRIB_AB_MASK)
  {
    case PLL_ATTRIB_AB_LEWIS: return -(double)p->pattern_weight_sum * log1p(-exp(mx) * sum);
    case PLL_ATTRIB_AB_FELSENSTEIN: return (double)wsum * (mx + log(sum));
    case PLL_ATTRIB_AB_STAMATAKIS:
      for (unsigned k = 0; k < S; ++k) corr += (double)w[k] * l[k];
      return corr;
    default: return 0.0;
  }
}

// first and second derivative of the correction from {A, B, C, count} of the constant patterns
static void asc_derivatives(const pll_partition_t * p, const double * abc, double * d1, double * d2)
{
  const unsigned S = p->states;
  const unsigned * w = p->pattern_weights + p->sites;
  unsigned mn = ~0u, wsum = 0;
  double a = 0.0, b = 0.0, c = 0.0;
  *d1 = *d2 = 0.0;
  for (unsigned k = 0; k < S; ++k) { mn = std::min(mn, (unsigned)abc[4 * k + 3]); wsum += w[k]; }
  for (unsigned k = 0; k < S; ++k)
  {
    const unsigned d = (unsigned)abc[4 * k + 3] - mn;
    const double f = (d == 0) ? 1.0 : (d <= 3) ? ldexp(1.0, -256 * (int)d) : 0.0;
    a += f * abc[4 * k]; b += f * abc[4 * k + 1]; c += f * abc[4 * k + 2];
  }
  switch (p->attributes & PLL_ATTRIB_AB_MASK)
  {
    case PLL_ATTRIB_AB_LEWIS:
    {
      const double t = (mn == 0) ? 1.0 : (mn <= 3) ? ldexp(1.0, -256 * (int)mn) : 0.0;
      const double q = t * b / (1.0 - t * a);
      *d1 = (double)p->pattern_weight_sum * q;
      *d2 = (double)p->pattern_weight_sum * (t * c / (1.0 - t * a) + q * q);
      break;
    }
    case PLL_ATTRIB_AB_FELSENSTEIN:
      *d1 = (double)wsum * (b / a);
      *d2 = (double)wsum * (c / a - (b / a) * (b / a));
      break;
    case PLL_ATTRIB_AB_STAMATAKIS:
      for (unsigned k = 0; k < S; ++k)
      {
        const double r1 = abc[4 * k + 1] / abc[4 * k], r2 = abc[4 * k + 2] / abc[4 * k];
        *d1 += (double)w[k] * r1;
        *d2 += (double)w[k] * (r2 - r1 * r1);
      }
      break;
    default: break;
  }
}

// Scalar results.  A reduction launch leaves its totals in the engine's current sink
// (Engine::sink): by default the pinned, device-mapped result buffer, whose sequence word
// the host polls; a deferred result (pllhip_results_*) points the sink at a device slot.
static void sink_to_host(Engine * e)
{
  e->sink.dst = e->d_result;
  e->sink.flag = reinterpret_cast<unsigned long long *>(e->d_result) + RESULT_SEQ_SLOT;
  e->sink.seq = ++e->result_seq;
}

// after the reduction kernel: the two-launch form adds the block totals in a second,
// single-block kernel; the fused form has nothing left to launch
static int finish_launch(Engine * e, unsigned nblocks, unsigned n_quant)
{
  if (e->fused_finish) return PLL_SUCCESS;
  hipLaunchKernelGGL(k_final_sum, dim3(1), dim3(256), 0, e->stream, reduce_out(e), nblocks, n_quant);
  PLLHIP_TRY(hipGetLastError());
  return PLL_SUCCESS;
}

// wait until the host sees sequence number `seq` in `flag` (mapped memory): poll for a short
// while -- scalar-returning calls are latency-bound for small slices (Newton-Raphson: a
// 14 us kernel per call) -- then fall back to a blocking stream synchronisation.
// PLLHIP_SPIN_US=0 disables the polling.
int wait_sequence(hipStream_t stream, const volatile unsigned long long * flag, unsigned long long seq, double timeout_s)
{
  static const long spin_us = getenv("PLLHIP_SPIN_US") ? atol(getenv("PLLHIP_SPIN_US")) : 400;
  bool done = false;
  const auto t0 = std::chrono::steady_clock::now();
  if (spin_us > 0)
  {
    for (unsigned it = 0; !done; ++it)
    {
      if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) done = true;
      else if ((it & 63u) == 63u &&
               std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > spin_us)
        break;
    }
  }
  if (!done && timeout_s > 0.0)
  {
    // a result another rank contributes to (a collective sits in front of it): never block without a bound --
    // a peer that died leaves the collective's kernel spinning for ever.  Poll the stream and the flag.
    for (;;)
    {
      if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return PLL_SUCCESS;
      const hipError_t q = hipStreamQuery(stream);
      if (q == hipSuccess) break;                      // the stream has drained: the flag decides below
      if (q != hipErrorNotReady) { (void)hip_ok(q, "hipStreamQuery"); return PLL_FAILURE; }
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
      {
        set_error(PLL_ERROR_HIP_TIMEOUT, "no result after %.1f s: a collective did not complete (peer lost?)", timeout_s);
        return PLL_FAILURE;
      }
      struct timespec ts = {0, 50000};
      nanosleep(&ts, nullptr);
    }
  }
  else if (!done) PLLHIP_TRY(hipStreamSynchronize(stream));
  if (!done && __atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq)
  {
    set_error(PLL_ERROR_HIP_RUNTIME, "a reduction finished without publishing its result");
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

static int finish_reduction(Engine * e, unsigned nblocks, unsigned n_quant, double * out)
{
  if (!finish_launch(e, nblocks, n_quant)) return PLL_FAILURE;
  const volatile unsigned long long * flag =
      reinterpret_cast<const volatile unsigned long long *>(e->h_result) + RESULT_SEQ_SLOT;
  if (!wait_sequence(e->stream, flag, e->sink.seq)) return PLL_FAILURE;
  for (unsigned q = 0; q < n_quant; ++q) out[q] = e->h_result[q];
  return PLL_SUCCESS;
}

static double * sumtable_device(Engine * e, const void * key, bool create)
{
  for (auto it = e->sumtables.begin(); it != e->sumtables.end(); ++it)
    if (it->first == key)
    {
      e->sumtables.splice(e->sumtables.begin(), e->sumtables, it);   // most recently used first
      return e->sumtables.front().second;
    }
  if (!create) return nullptr;
  double * buf = nullptr;
  if (e->sumtables.size() >= MAX_SUMTABLES)
  {
    // recycle the least recently used table (same size for every key)
    buf = e->sumtables.back().second;
    e->sumtables.pop_back();
  }
  else if (!dev_alloc(&buf, e->clv_len, "sumtable"))
    return nullptr;
  e->sumtables.emplace_front(key, buf);
  return buf;
}

static int check_clv_index(const Engine * e, unsigned idx, const char * what)
{
  if (idx >= e->nodes)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s CLV index %u out of range", what, idx);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

static int check_scaler_index(const Engine * e, int idx)
{
  if (idx != PLL_SCALE_BUFFER_NONE && (idx < 0 || (unsigned)idx >= e->nscalers))
  {
    set_error(PLL_ERROR_PARAM_INVALID, "scaler index %d out of range", idx);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

// ---------------------------------------------------------------------------
// The families with operation chains (4 states, 2 .. 32 states, 20 states): what the schedules of
// pll_update_partials and pllhip_update_partials_batch and the class nodes of site repeats need of one.
// chain_family() is the one place of that path that tells the families apart.
// ---------------------------------------------------------------------------
struct ChainFamily
{
  bool (*supported)(const Engine * e);                  // chains at the partition's rates, scaling and tip tables
  unsigned chain_max;                                   // operations per chain
  unsigned chain_lds;                                   // LDS doubles of one chain's tables (~0u: no limit)
  // DevicePlan::lds_doubles and the LDS argument of `traverse` / `chains`: the doubles of the largest chain's tables
  // (child_lds / wide_lds summed over its operations) -- or, with lds_is_length, the operations of the longest chain
  // (4 states: every link has an area of the same size, s4_chain_op_lds)
  bool lds_is_length;
  unsigned (*extent)(const Engine * e);                 // PlanChain::extent: sites (4 states) or site blocks
  unsigned (*child_lds)(const Engine * e, bool tip, unsigned lut_used);   // LDS doubles of a child's table in a chain
  // ... of a wide tip with `rows` classes (a class node read through its row table, kernels_repeats.hpp): staged when
  // they take no more than a coded tip's table may, else gathered from memory (0)
  unsigned (*wide_lds)(const Engine * e, unsigned rows);
  bool (*tables_in_lds)(const Engine * e, unsigned lut_used);             // PlanChain::flags bit 0
  // the family folds lone cherries into the chain that reads them (plan_folds): LDS doubles of one fold in its
  // consumer's chain (null: the family has no folds; 0: none at this partition's shape)
  unsigned (*fold_lds)(const Engine * e, unsigned lut_used);
  // the family reads small light subtrees through class tables (plan_lookups): the most classes of such a child
  // (null: the family has no such reads; 0: none at this partition's shape)
  unsigned (*look_classes)(const Engine * e, unsigned lut_used);
  // the family's storing schedules leave out the stores nobody reads (plan_defers; null: never; level 0: not at this
  // partition's shape; DeferPolicy, chain_plan.hpp)
  DeferPolicy (*defer)(const Engine * e);
  const double * (*pair_pfrag)(const Engine * e, unsigned matrix);        // PairLutJob::pfrag of a branch
  bool (*fills_chip)(const Engine * e);                 // the site blocks alone keep the chip busy: one launch
  unsigned (*units)(const Engine * e);                  // workgroups a member of a batch can use side by side
  unsigned batch_wgs;                                   // workgroups per CU and row of a batch in one launch
  // a resident schedule (DevicePlan, upload_plan): chains [begin, end) in `rows` grid rows
  int (*traverse)(Engine * e, const PlanView & view, unsigned lds_doubles, unsigned extent, unsigned begin,
                  unsigned end, unsigned rows, unsigned wgs, bool wide, bool transient, bool fold, bool look);
  // chains by value in the kernel arguments (null: none)
  int (*chains)(Engine * e, const ChainBatch & batch, unsigned nchains, unsigned lds, unsigned lut_used);
  // class nodes (kernels_repeats.hpp): row tables, class tables, the site-indexed vector of one node
  void (*pair_lut)(Engine * e, const PairLutJob * jobs, unsigned njobs, unsigned max_rows);
  void (*class_build)(Engine * e, const CherryJob * jobs, unsigned njobs, unsigned max_classes, unsigned ncodes);
  void (*class_expand)(Engine * e, const Engine::Cherry & c, double * out);
};

// 20 states: the most classes of a light child that its consumer reads through the child's class table.  Default: a
// cherry (U^2 classes for U codes in use) and a cherry x tip (U^3); PLLHIP_LOOKUP_CLASSES sets another limit.  Two
// class codes share a register in the kernel (S20_LOOK_MAX).
// The read pays where the child's vector would come back from HBM.  A partition small enough for the one-launch
// traversal reads it from the caches (its wave wrote it a few chains ago), and there the gather and the table launches
// only cost (C3's 125 k-site slice: 4.09 -> 4.25 ms per traversal, against 28.19 -> 27.62 ms at 1 M sites): a floor
// of S20_LOOK_MIN_BLOCKS site blocks.  PLLHIP_LOOKUP=1 plans the reads at any size, PLLHIP_LOOKUP=0 at none.
constexpr unsigned S20_LOOK_MIN_BLOCKS = 8192;          // 262 144 sites
static unsigned s20_look_classes(const Engine * e, unsigned lut_used)
{
  static const int use_look = getenv("PLLHIP_LOOKUP") ? atoi(getenv("PLLHIP_LOOKUP")) : -1;
  static const long env_classes = getenv("PLLHIP_LOOKUP_CLASSES") ? atol(getenv("PLLHIP_LOOKUP_CLASSES")) : -1;
  if (!use_look || !e->d_pfrag || (use_look < 0 && e->nblk < S20_LOOK_MIN_BLOCKS)) return 0u;
  const unsigned long long limit = env_classes >= 0 ? (unsigned long long)env_classes
                                                    : (unsigned long long)lut_used * lut_used * lut_used;
  return (unsigned)std::min<unsigned long long>(limit, S20_LOOK_MAX);
}

// 20 states: whether a storing schedule leaves out the stores nobody reads (plan_defers): 0 = no, 1 = those of folded
// cherries and of looked-up children, 2 = those of folded cherries alone, 3 = level 1 and the tip-only runs at the
// bottom of the chains, 4 = level 3 and the vectors inside the chains; depth (level 3): the most operations of
// such a run that are left out (0: the whole run).  A store
// that is made up for later costs a launch of its own on top of its bytes, which a small partition never saved in the
// traversal: a floor of S20_DEFER_MIN_BLOCKS site blocks, just under the smallest partition measured to gain (C3's
// 125 k-site slice, 3 907 blocks: 4.07 -> 3.96 ms per evaluation).  PLLHIP_DEFER=1 / 3 / 4 defers at any size (the
// tests do), PLLHIP_DEFER=0 at none (every vector is stored by the traversal that computes it: the reference of the A/B
// runs and of the bitwise tests), PLLHIP_DEFER=2 defers the folded half alone, at any size (the A/B runs that weigh the
// two halves separately).  PLLHIP_DEFER_DEPTH=D caps the runs of level 3 at D operations (0: no cap); level 4 = level 3
// and every vector inside a chain that the next operation takes in registers and nobody reads from memory, without a cap.
// Without PLLHIP_DEFER the level follows what the caller does with the vectors that were left out (DESIGN.md sections
// 22 and 26): a higher level gains on an evaluation that is followed by another evaluation, and costs an evaluation that
// is followed by a pass over all branches more than it saved.  So level 1 is planned until S20_DEFER_RUN_ROW lists in a
// row that left stores out have come and gone without one deferred vector being stored later (UnstoredLedger::unread_row,
// run_resident), level 3 from then on, level 4 once S20_DEFER_CHAIN_ROW such lists have, and level 1 again as soon as a
// reader asks for a deferred vector.  S20_DEFER_CHAIN_ROW = max(4, ceil(T / G)) at the size where T / G is largest: G is
// what level 4 gains per evaluation over level 3, T what the turn "evaluation, then a pass over all branches" costs more
// at level 4 than at level 3, plus G.  Measured on C3 (section 26; medians of three processes, ms):
//   125 000 sites  G 0.61  T 1.50  T / G 2.5;  250 000 sites  G 0.92  T 2.72  T / G 3.0;  500 000 sites  G 1.91  T 5.56  T / G 2.9
// so ceil(T / G) = 3 and the bound of 4 decides: a caller who reads after a row of evaluations has by then saved more
// than the turn costs, and a row of fewer than five evaluations never reaches level 4.  The 125 k-site slice gains
// (3.42 -> 2.81 ms per evaluation), so level 4 shares the floor.
constexpr unsigned S20_DEFER_MIN_BLOCKS = 3840;         // 122 880 sites
constexpr unsigned S20_DEFER_DEPTH = 0;                 // without PLLHIP_DEFER_DEPTH
constexpr unsigned S20_DEFER_RUN_ROW = 2;               // unread lists in a row before level 3
constexpr unsigned S20_DEFER_CHAIN_ROW = 4;             // ... before level 4
static DeferPolicy s20_defer(const Engine * e)
{
  static const int use_defer = getenv("PLLHIP_DEFER") ? atoi(getenv("PLLHIP_DEFER")) : -1;
  static const int env_depth = getenv("PLLHIP_DEFER_DEPTH") ? atoi(getenv("PLLHIP_DEFER_DEPTH")) : -1;
  if (!use_defer || (use_defer < 0 && e->nblk < S20_DEFER_MIN_BLOCKS)) return {};
  // (the lists in a row that went unread so far; a vector stored since the last of them ends the row)
  const unsigned row = e->ledger.unread_row();
  const unsigned level = use_defer < 0 ? (row >= S20_DEFER_CHAIN_ROW ? 4u : row >= S20_DEFER_RUN_ROW ? 3u : 1u)
                       : use_defer == 2 ? 2u : use_defer == 3 ? 3u : use_defer >= 4 ? 4u : 1u;
  const unsigned depth = env_depth < 0 ? S20_DEFER_DEPTH : (unsigned)std::min(env_depth, 1023);
  return {level, level == 3 ? depth : 0u};
}

static const ChainFamily CHAINS_S4 = {
  .supported = chains_supported_s4, .chain_max = S4_CHAIN_MAX, .chain_lds = ~0u, .lds_is_length = true,
  .extent = [](const Engine * e) { return e->N; },
  .child_lds = [](const Engine *, bool, unsigned) { return 0u; },
  .wide_lds = [](const Engine *, unsigned) { return 0u; },
  .tables_in_lds = [](const Engine *, unsigned) { return false; },
  .fold_lds = nullptr, .look_classes = nullptr, .defer = nullptr,
  .pair_pfrag = [](const Engine * e, unsigned m) -> const double * { return e->d_pmat + (size_t)m * e->R * 16; },
  .fills_chip = [](const Engine * e) { return (e->N + 63) / 64 >= 48u * e->cu_count; },
  .units = [](const Engine * e) { return (e->N + 255u) / 256u; }, .batch_wgs = 3,
  .traverse = launch_traverse_s4, .chains = launch_chains_s4,
  .pair_lut = [](Engine * e, const PairLutJob * jobs, unsigned njobs, unsigned max_rows)
  { hipLaunchKernelGGL(k_pair_lut_s4, dim3((max_rows * e->R + 255) / 256, njobs), dim3(256), 0, e->stream, jobs, e->R); },
  .class_build = [](Engine * e, const CherryJob * jobs, unsigned njobs, unsigned max_classes, unsigned ncodes)
  { hipLaunchKernelGGL(k_cherry_build_s4, dim3((max_classes + 255) / 256, njobs), dim3(256), 0, e->stream, jobs, e->R, ncodes); },
  .class_expand = [](Engine * e, const Engine::Cherry & c, double * out)
  {
    hipLaunchKernelGGL(k_cherry_expand_s4, dim3(std::max(1u, std::min((e->N * e->R + 255u) / 256u, e->cu_count * 8u))), dim3(256), 0,
                       e->stream, c.table, c.pair, e->N, e->R, out);
  },
};

static const ChainFamily CHAINS_S16 = {
  .supported = chains_supported_s16, .chain_max = S16_CHAIN_MAX, .chain_lds = S16_CHAIN_LDS, .lds_is_length = false,
  .extent = [](const Engine * e) { return e->nblk; },
  .child_lds = [](const Engine * e, bool tip, unsigned) { return s16_chain_slot(e, tip); },
  .wide_lds = [](const Engine * e, unsigned rows) { return e->R * rows * e->S <= S16_LUT_LDS ? ((e->R * rows * e->S + 7u) & ~7u) : 0u; },
  .tables_in_lds = [](const Engine * e, unsigned) { return s16_chain_lut_lds(e); },
  .fold_lds = nullptr, .look_classes = nullptr, .defer = nullptr,
  .pair_pfrag = [](const Engine * e, unsigned m) -> const double * { return e->d_pmat + (size_t)m * e->R * e->S * e->Sp; },
  .fills_chip = [](const Engine * e) { return e->nblk >= 12u * e->cu_count && e->nblk < 48u * e->cu_count && e->S > 8; },
  .units = [](const Engine * e) { return (e->nblk + 7u) / 8u; }, .batch_wgs = 1,
  .traverse = launch_traverse_s16, .chains = nullptr,        // (chains exist in the resident form only)
  .pair_lut = [](Engine * e, const PairLutJob * jobs, unsigned njobs, unsigned max_rows)
  {
    const dim3 gp(((max_rows + S20_BS - 1) / S20_BS + 3) / 4, njobs);
#define PLLHIP_CALL(KK) \
    hipLaunchKernelGGL(k_pair_lut_s16<KK>, gp, dim3(256), sizeof(double) * e->R * s16_fr(KK), e->stream, jobs, e->R, e->S, e->Sp)
    PLLHIP_DISPATCH_KS(s16_ks(e), PLLHIP_CALL);
#undef PLLHIP_CALL
  },
  .class_build = [](Engine * e, const CherryJob * jobs, unsigned njobs, unsigned max_classes, unsigned ncodes)
  {
    const dim3 gb(((max_classes + S20_BS - 1) / S20_BS + 3) / 4, njobs);
#define PLLHIP_CALL(KK) hipLaunchKernelGGL(k_cherry_build_s16<KK>, gb, dim3(256), 0, e->stream, jobs, ncodes, e->R, e->S)
    PLLHIP_DISPATCH_KS(s16_ks(e), PLLHIP_CALL);
#undef PLLHIP_CALL
  },
  .class_expand = [](Engine * e, const Engine::Cherry & c, double * out)
  {
#define PLLHIP_CALL(KK) \
    hipLaunchKernelGGL(k_cherry_expand_s16<KK>, dim3(std::max(1u, std::min((e->nblk + 3) / 4, e->cu_count * 8u))), dim3(256), 0, \
                       e->stream, c.table, c.pair, e->nblk, e->R, out)
    PLLHIP_DISPATCH_KS(s16_ks(e), PLLHIP_CALL);
#undef PLLHIP_CALL
  },
};

static const ChainFamily CHAINS_S20 = {
  .supported = chains_supported_s20, .chain_max = S20_CHAIN_MAX, .chain_lds = S20_CHAIN_LDS, .lds_is_length = false,
  .extent = [](const Engine * e) { return e->nblk; },
  .child_lds = s20_chain_slot,
  .wide_lds = [](const Engine * e, unsigned rows) { return e->R * rows * S20_LUT_RS <= 2560u ? ((e->R * rows * S20_LUT_RS + 7u) & ~7u) : 0u; },
  .tables_in_lds = s20_chain_lut_lds,
  .fold_lds = s20_fold_lds, .look_classes = s20_look_classes, .defer = s20_defer,
  .pair_pfrag = [](const Engine * e, unsigned m) -> const double * { return e->d_pfrag + (size_t)m * e->R * 400; },
  .fills_chip = [](const Engine * e) { return e->nblk >= 6u * e->cu_count && e->nblk < 24u * e->cu_count; },
  .units = [](const Engine * e) { return (e->nblk + 7u) / 8u; }, .batch_wgs = 1,
  .traverse = launch_traverse_s20, .chains = launch_chains_s20,
  .pair_lut = [](Engine * e, const PairLutJob * jobs, unsigned njobs, unsigned max_rows)
  {
    const dim3 gp(((max_rows + S20_BS - 1) / S20_BS + 3) / 4, njobs);
    const size_t lds = sizeof(double) * e->R * S20_CFRAGS;
    if (e->R == 4) hipLaunchKernelGGL(k_pair_lut<4>, gp, dim3(256), lds, e->stream, jobs);
    else if (e->R == 2) hipLaunchKernelGGL(k_pair_lut<2>, gp, dim3(256), lds, e->stream, jobs);
    else hipLaunchKernelGGL(k_pair_lut<1>, gp, dim3(256), lds, e->stream, jobs);
  },
  .class_build = [](Engine * e, const CherryJob * jobs, unsigned njobs, unsigned max_classes, unsigned ncodes)
  {
    const dim3 gb(((max_classes + S20_BS - 1) / S20_BS + 3) / 4, njobs);
    if (e->R == 4) hipLaunchKernelGGL(k_cherry_build<4>, gb, dim3(256), 0, e->stream, jobs, ncodes);
    else if (e->R == 2) hipLaunchKernelGGL(k_cherry_build<2>, gb, dim3(256), 0, e->stream, jobs, ncodes);
    else hipLaunchKernelGGL(k_cherry_build<1>, gb, dim3(256), 0, e->stream, jobs, ncodes);
  },
  .class_expand = [](Engine * e, const Engine::Cherry & c, double * out)
  {
    hipLaunchKernelGGL(k_cherry_expand, dim3(std::max(1u, std::min((e->nblk + 3) / 4, e->cu_count * 8u))), dim3(256), 0,
                       e->stream, c.table, c.pair, e->nblk, e->R, out);
  },
};

// the family's entry whatever the partition's shape (class nodes exist for these families only)
static const ChainFamily * family_entry(KernelFamily f)
{
  return f == KernelFamily::S4 ? &CHAINS_S4 : f == KernelFamily::S16 ? &CHAINS_S16 : f == KernelFamily::S20 ? &CHAINS_S20
                                                                                                          : nullptr;
}

// the chains of this partition, or null: none in its family or at its shape, or PLLHIP_CHAINS=0 (the plain level
// schedule)
static const ChainFamily * chain_family(const Engine * e)
{
  static const int use_chains = getenv("PLLHIP_CHAINS") ? atoi(getenv("PLLHIP_CHAINS")) : 1;
  const ChainFamily * f = family_entry(e->family);
  return use_chains && f && f->supported(e) ? f : nullptr;
}

// ---------------------------------------------------------------------------
// The edge path (edge and root lnL, sumtable, derivatives, the device Newton-Raphson loop): what it needs of a kernel
// family.  Every partition has an entry, the generic family included; edge_family() is the one place of this path that
// tells the families apart.
// ---------------------------------------------------------------------------
static bool newton_probe_s4(Engine * e), newton_probe_s16(Engine * e), newton_probe_s20(Engine * e), newton_probe_s61(Engine * e);

struct EdgeFamily
{
  const char * name;                                    // pllhip_partials_kernel_name
  int (*partials)(Engine * e, const OpBatch & batch, unsigned nops);     // one level of the plain schedule
  // lnL at an edge, and at a root vector (pm, lut null; k_edge_lnl_s4 has no root form: 4 states take the generic kernel)
  int (*lnl)(Engine * e, const ModelView & mv, const ParamIdx & fidx, const NodeRef & parent, const NodeRef & child,
             const double * pm, const double * lut, const unsigned * ps, const unsigned * cs, double * persite, unsigned nblocks);
  decltype(lnl) root_lnl;
  bool root_child_scaler;                               // the root form is handed the caller's child scaler (else none)
  int (*sumtable)(Engine * e, const ModelView & mv, const ParamIdx & params, const NodeRef & parent, const NodeRef & child,
                  double * d_sum);
  int (*derivatives)(Engine * e, const ModelView & mv, const ParamIdx & params, const TrialLengths & tl, unsigned count,
                     const double * d_sum, const unsigned * ps, const unsigned * cs, unsigned nblocks);
  // reduce_grid(): the workgroups that have work -- one thread per site (generic), one lane per (site, rate) and 4 per
  // trip (4 states), one wave per site block (blocked families) -- and the most that are launched
  unsigned long long (*reduce_need)(const Engine * e);
  unsigned reduce_cap;
  bool scan_on_newton_grid;                             // derivative scans run on scan_grid(), not on reduce_grid()
  // trial lengths per derivatives launch: four on the matrix cores; the others are bounded by their coefficient tables
  // (3 x R x S doubles per length, below 48 KiB of LDS).  0: no launch carries this shape (error set)
  unsigned (*trial_lengths)(const Engine * e);
  // the device Newton-Raphson loop.  newton_probe fills the engine's newton_* cache once (false: HIP error; nothing is
  // cached, unless it was the resident candidate's query that failed: the streaming loop stays); null: no loop kernel
  // (the three newton_* entries below are null with it: newton_prepare and the newton_kind test at the top of
  // newton_multi_one_launch turn such a partition away before anything reads them)
  bool (*newton_probe)(Engine * e);
  bool newton_rate_scalers;                             // ... that handles per-rate scalers
  unsigned (*newton_ks)(const Engine * e);              // k-steps of the matrix-core loop (0: none, the 4-state loop)
  unsigned (*newton_kind)(const Engine * e);            // NewtonMultiPart::kind
};

// LDS of the streaming matrix-core loop, and of a partition's part in k_newton_multi
static size_t newton_table_lds(const Engine * e, unsigned ks) { return sizeof(double) * e->R * ks * 64; }

static unsigned long long reduce_need_blocked(const Engine * e) { return ((unsigned long long)e->nblk + 3ULL) / 4ULL; }
static unsigned trial_lengths_blocked(const Engine *) { return 4u; }

static const EdgeFamily EDGE_GENERIC = {
  .name = "generic", .partials = launch_partials_generic,
  .lnl = launch_edge_lnl_generic, .root_lnl = launch_edge_lnl_generic, .root_child_scaler = false,
  .sumtable = launch_sumtable_generic, .derivatives = launch_derivatives_generic,
  .reduce_need = [](const Engine * e) { return ((unsigned long long)e->N + 255ULL) / 256ULL; }, .reduce_cap = 2048,
  .scan_on_newton_grid = false,
  .trial_lengths = [](const Engine * e)
  {
    unsigned kmax = MAX_TRIAL_LENGTHS;
    while (kmax > 1 && (size_t)3 * kmax * e->R * e->S * sizeof(double) > 48 * 1024) kmax >>= 1;
    if ((size_t)3 * e->R * e->S * sizeof(double) <= 64 * 1024) return kmax;
    set_error(PLL_ERROR_PARAM_INVALID, "derivatives: %u rates x %u states exceed the LDS tables", e->R, e->S);
    return 0u;
  },
  .newton_probe = nullptr, .newton_rate_scalers = false, .newton_ks = nullptr, .newton_kind = nullptr,
};

static const EdgeFamily EDGE_S4 = {
  .name = "s4-valu", .partials = launch_partials_s4,
  .lnl = launch_edge_lnl_s4, .root_lnl = launch_edge_lnl_generic, .root_child_scaler = false,
  .sumtable = launch_sumtable_s4, .derivatives = launch_derivatives_s4,
  .reduce_need = [](const Engine * e) { return ((unsigned long long)e->N * e->R + 1023ULL) / 1024ULL; }, .reduce_cap = 1024,
  .scan_on_newton_grid = true, .trial_lengths = [](const Engine *) { return MAX_TRIAL_LENGTHS; },
  .newton_probe = newton_probe_s4, .newton_rate_scalers = false, .newton_ks = [](const Engine *) { return 0u; },
  .newton_kind = [](const Engine *) { return NEWTON_KIND_S4; },
};

static const EdgeFamily EDGE_S16 = {
  .name = "s16-mfma",
  .partials = [](Engine * e, const OpBatch & batch, unsigned nops) { return launch_partials_s16(e, batch, nops); },
  .lnl = launch_edge_lnl_s16, .root_lnl = launch_edge_lnl_s16, .root_child_scaler = false,
  .sumtable = launch_sumtable_s16, .derivatives = launch_derivatives_s16,
  .reduce_need = reduce_need_blocked, .reduce_cap = 2048, .scan_on_newton_grid = true, .trial_lengths = trial_lengths_blocked,
  .newton_probe = newton_probe_s16, .newton_rate_scalers = true, .newton_ks = s16_ks,
  .newton_kind = [](const Engine * e) { return NEWTON_KIND_S16 + s16_ks(e) - 1; },
};

static const EdgeFamily EDGE_S20 = {
  .name = "s20-mfma", .partials = launch_partials_s20,
  .lnl = launch_edge_lnl_s20, .root_lnl = launch_edge_lnl_s20, .root_child_scaler = true,
  .sumtable = launch_sumtable_s20, .derivatives = launch_derivatives_s20,
  .reduce_need = reduce_need_blocked, .reduce_cap = 2048, .scan_on_newton_grid = true, .trial_lengths = trial_lengths_blocked,
  .newton_probe = newton_probe_s20, .newton_rate_scalers = true, .newton_ks = [](const Engine *) { return 5u; },
  .newton_kind = [](const Engine *) { return NEWTON_KIND_S20; },
};

static const EdgeFamily EDGE_S61 = {
  .name = "s61-mfma", .partials = launch_partials_s61,
  .lnl = launch_edge_lnl_s61, .root_lnl = launch_edge_lnl_s61, .root_child_scaler = true,
  .sumtable = launch_sumtable_s61, .derivatives = launch_derivatives_s61,
  .reduce_need = reduce_need_blocked, .reduce_cap = 2048, .scan_on_newton_grid = true, .trial_lengths = trial_lengths_blocked,
  .newton_probe = newton_probe_s61, .newton_rate_scalers = true, .newton_ks = [](const Engine *) { return S61_KS; },
  .newton_kind = [](const Engine * e) { return e->S == S61_S ? NEWTON_KIND_S61 : NEWTON_KIND_S61_RT; },
};

static const EdgeFamily * edge_family(const Engine * e)
{
  switch (e->family)
  {
    case KernelFamily::S4: return &EDGE_S4;
    case KernelFamily::S16: return &EDGE_S16;
    case KernelFamily::S20: return &EDGE_S20;
    case KernelFamily::S61: return &EDGE_S61;
    default: return &EDGE_GENERIC;
  }
}

static int launch_partials(Engine * e, const OpBatch & batch, unsigned nops) { return edge_family(e)->partials(e, batch, nops); }

static unsigned reduce_grid(const Engine * e)
{
  const EdgeFamily * f = edge_family(e);
  // fewer, longer-lived workgroups than one per trip: their prologue (matrix / fragment loads)
  // and the block reduction are paid less often (measured at 1 M sites: 4-state lnL 82 -> 62 us
  // with 1024 blocks, 20-state lnL 254 -> 245 us with 2048)
  static const unsigned env_cap = getenv("PLLHIP_REDUCE_BLOCKS") ? (unsigned)atoi(getenv("PLLHIP_REDUCE_BLOCKS")) : 0u;
  const unsigned cap = env_cap ? env_cap : f->reduce_cap;
  return (unsigned)std::max<unsigned long long>(1ULL, std::min<unsigned long long>(f->reduce_need(e), std::min(cap, (unsigned)REDUCE_BLOCKS)));
}

// a tip that is read through byte codes and the partition's lookup tables (PLL_ATTRIB_PATTERN_TIP); without the
// attribute a tip is a vector -- and, when it came through pll_set_tip_states, a class node as well (upload_tip_classes)
static bool coded_tip(const Engine * e, unsigned idx) { return e->coded_tips && idx < e->tips; }

// LDS doubles of a lone cherry folded into the chain that reads it, or 0: the family has no folds, none at this
// shape, or PLLHIP_FOLD=0 (the schedules without folds: the reference of the A/B runs and of the bitwise tests)
static unsigned fold_table_lds(const Engine * e, const ChainFamily & f, unsigned lut_used)
{
  static const int use_fold = getenv("PLLHIP_FOLD") ? atoi(getenv("PLLHIP_FOLD")) : 1;
  return use_fold && f.fold_lds && e->coded_tips ? f.fold_lds(e, lut_used) : 0u;
}

// whether a storing schedule with folds leaves out the stores nobody reads (plan_defers; the family says which and
// from what size on: ChainFamily::defer)
static DeferPolicy defer_stores(const Engine * e, const ChainFamily & f, bool transient)
{
  // (an evaluate-only traversal leaves these vectors out already; the lists that store vectors later store them)
  if (!f.defer || transient || e->transient_mode || e->transient_busy || e->site_repeats) return {};
  return f.defer(e);
}

// LDS doubles of the table of child `idx` in a chain kernel; wide: the child is read as a wide tip
static unsigned child_table_lds(const Engine * e, const ChainFamily & f, unsigned idx, unsigned lut_used, bool wide)
{
  return wide ? f.wide_lds(e, e->cherries[idx].nclasses) : f.child_lds(e, coded_tip(e, idx), lut_used);
}

// An operation list as the chain planner takes it (chain_plan.hpp: the planner knows nothing of the engine), and what
// its one pass over the list found.  accepted: the list has the shape of a tree traversal; anything else keeps the
// level schedule.
// f: the family whose tables count against the LDS cap (null: no tables, the shape alone)
// wide: [2 * count] which children are read as wide tips (null or empty: none)
struct PlannedList
{
  std::vector<unsigned> costs;                   // per child: child_table_lds
  ChainList list;
  ListFacts facts;
  bool accepted;
  PlannedList(const Engine * e, const ChainFamily * f, const pll_operation_t * ops, unsigned count, unsigned lut_used,
              const std::vector<unsigned char> * wide = nullptr)
  {
    const bool w = wide && !wide->empty();
    costs.resize(f ? 2 * (size_t)count : 0);
    for (size_t i = 0; i < costs.size(); ++i)
      costs[i] = child_table_lds(e, *f, i & 1 ? ops[i / 2].child2_clv_index : ops[i / 2].child1_clv_index, lut_used, w && (*wide)[i]);
    list = {ops, count, e->nodes, e->nscalers, e->coded_tips ? e->tips : 0u, f ? costs.data() : nullptr};
    accepted = analyse_list(list, facts);
  }
  PlannedList(const PlannedList &) = delete;
};

// bytes in Engine::d_looktab of the tables of one looked-up child (ChainPlan::lookups, reserve_lookup_tables): [0] top,
// [1] the cherry below it
struct LookupRoom
{
  size_t off_table[2], off_flags[2], off_counts[2], off_rows[2];
};

// make DevicePlan::bytes resident on the device (stream-ordered; nothing is copied when the
// device already holds exactly these bytes) and point `view` at it
static int upload_plan(DevicePlan & dp, hipStream_t stream, PlanView & view)
{
  const size_t len = dp.bytes.size();
  // a few operations without class jobs: in the kernel arguments (no copy in front of the launch: PlanView, engine.h)
  // (only where the kernel arguments live in device memory -- HIP_FORCE_DEV_KERNARG=1, which the library asks for when it
  // is loaded --: the kernels re-read their entries per site block, and those reads should not cross the bus)
  static const int env_inline = getenv("PLLHIP_PLAN_INLINE") ? atoi(getenv("PLLHIP_PLAN_INLINE"))
                              : (getenv("HIP_FORCE_DEV_KERNARG") && atoi(getenv("HIP_FORCE_DEV_KERNARG")) == 1 ? 1 : 0);
  if (env_inline && len <= PLAN_INLINE_BYTES && dp.nops && !dp.ncherry_jobs && !dp.npair_jobs &&
      len == (size_t)dp.nops * sizeof(PlanOp) + (size_t)dp.nchains * sizeof(PlanChain))
  {
    memset(&view, 0, sizeof(view));
    memcpy(view.inl, dp.bytes.data(), len);
    view.inline_ops = dp.nops * (unsigned)sizeof(PlanOp);
    view.nchains = dp.nchains;
    return PLL_SUCCESS;
  }
  view.inline_ops = 0;
  if (dp.resident != dp.bytes)
  {
    if (len > dp.cap)
    {
      PLLHIP_TRY(hipStreamSynchronize(stream));    // a running traversal may still read the old buffer
      (void)hipFree(dp.d_buf);
      dp.d_buf = nullptr;
      dp.cap = 0;
      const size_t cap = std::max<size_t>(2 * len, 65536);
      if (!dev_alloc(&dp.d_buf, cap, "traversal schedule")) return PLL_FAILURE;
      dp.cap = cap;
    }
    if (!dp.copied) PLLHIP_TRY(hipEventCreateWithFlags(&dp.copied, hipEventDisableTiming));
    else PLLHIP_TRY(hipEventSynchronize(dp.copied));  // the previous upload has left the staging buffer
    if (len > dp.h_cap)
    {
      if (dp.h_stage) (void)hipHostFree(dp.h_stage);
      dp.h_stage = nullptr;
      dp.h_cap = 0;
      const size_t cap = std::max<size_t>(2 * len, 65536);
      PLLHIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&dp.h_stage), cap, hipHostMallocDefault));
      dp.h_cap = cap;
    }
    memcpy(dp.h_stage, dp.bytes.data(), len);
    PLLHIP_TRY(hipMemcpyAsync(dp.d_buf, dp.h_stage, len, hipMemcpyHostToDevice, stream));
    PLLHIP_TRY(hipEventRecord(dp.copied, stream));
    dp.resident = dp.bytes;
  }
  view.ops = reinterpret_cast<const PlanOp *>(dp.d_buf);
  view.chains = reinterpret_cast<const PlanChain *>(dp.d_buf + (size_t)dp.nops * sizeof(PlanOp));
  view.nchains = dp.nchains;
  return PLL_SUCCESS;
}

// ---------------------------------------------------------------------------
// site repeats (kernels_repeats.hpp): host side
// ---------------------------------------------------------------------------
// a reader needs the per-site counts of scale buffer `sidx`: written out if they exist per class only
static int need_scaler(Engine * e, int sidx)
{
  if (sidx < 0 || (size_t)sidx >= e->scaler_lazy.size() || e->scaler_lazy[sidx] < 0) return PLL_SUCCESS;
  const Engine::Cherry & c = e->cherries[e->scaler_lazy[sidx]];
  hipLaunchKernelGGL(k_class_scaler_expand, dim3(std::max(1u, std::min((e->Nalloc + 255u) / 256u, 4u * e->cu_count))), dim3(256), 0,
                     e->stream, (const unsigned *)c.counts, (const unsigned *)c.pair, e->Nalloc,
                     e->d_scalers + (size_t)sidx * e->sc_len);
  PLLHIP_TRY(hipGetLastError());
  e->scaler_lazy[sidx] = -1;
  return PLL_SUCCESS;
}

// a reader needs the site-indexed vector of `idx` (and the per-site counts that go with it): expand them if the node
// is kept per class
static int need_clv(Engine * e, unsigned idx)
{
  // (an evaluate-only traversal kept it in registers: recomputed and stored now)
  if (!e->ledger.empty() && !e->transient_busy && e->ledger.live(idx) &&
      !store_unstored(e, std::vector<unsigned>(1, idx))) return PLL_FAILURE;
  if (e->cherries.empty() || idx >= e->cherries.size()) return PLL_SUCCESS;
  Engine::Cherry & c = e->cherries[idx];
  if (c.valid && c.scaler_index >= 0 && (size_t)c.scaler_index < e->scaler_lazy.size() && e->scaler_lazy[c.scaler_index] == (int)idx &&
      !need_scaler(e, c.scaler_index)) return PLL_FAILURE;
  if (!c.valid || c.materialized) return PLL_SUCCESS;
  family_entry(e->family)->class_expand(e, c, e->d_clv[idx]);
  PLLHIP_TRY(hipGetLastError());
  c.materialized = true;
  e->repeat_stats.expansions++;
  return PLL_SUCCESS;
}

// which operations of a list the schedule keeps per class (cherries and the class nodes above them), and which
// children the others read as wide tips
struct RepeatPlan
{
  bool active = false;
  std::vector<pll_operation_t> ops;          // the list without the class operations
  std::vector<unsigned> cherry_ops;          // positions of the class operations in the original list (post-order)
  unsigned ncodes = 0;
};

// limits of the class numbering: pairs of child classes that go through a table of all possible pairs (libpll's
// PLL_REPEATS_LOOKUP_SIZE plays this role in pll_update_repeats; more pairs: a hash table of the pairs that occur, as
// long as its slots fit the prefix sum), and how much smaller than the alignment a class table has to be for the
// node to be worth it (the class pipeline writes and gathers rows per class child: no gain from about a third)
// (measured on one box, ms per traversal at ratio 16 / 8 / 4 / 3: C3 random 22.98 / 23.09 / 22.14 / 22.65, simulated
// 20.92 / 20.68 / 18.75 / 18.71; C2 random 1.976 / 1.973 / 1.990 / 2.115, simulated 1.864 / 1.857 / 2.019 / 2.191:
// the 128-byte vectors of 4 states leave less to win per site than the codes and counts of a class node cost)
constexpr unsigned long long CLASS_MAX_PAIRS = 1024ULL * 4096ULL;
constexpr unsigned CLASS_MIN_RATIO_S20 = 4u, CLASS_MIN_RATIO_S4 = 8u;

static bool cherry_storage(Engine * e, unsigned node, unsigned nclasses)
{
  Engine::Cherry & c = e->cherries[node];
  const unsigned npblk = (nclasses + S20_BS - 1) / S20_BS;
  // (20 states: blocked like a vector over the classes; 4 states: [class][rate][4])
  const size_t table_doubles = e->family == KernelFamily::S4 ? (size_t)nclasses * e->R * 4
                             : e->family == KernelFamily::S16 ? (size_t)npblk * e->R * 4 * s16_ks(e) * S20_BS
                                                               : (size_t)npblk * e->R * S20_UNIT;
  if (c.cap_classes < nclasses)
  {
    if (hipStreamSynchronize(e->stream) != hipSuccess) return false;
    (void)hipFree(c.table); (void)hipFree(c.flags); (void)hipFree(c.counts);
    c.table = nullptr; c.flags = nullptr; c.counts = nullptr; c.cap_classes = 0;
    e->plan.key.clear();                          // cached schedules point at the old tables
    if (!dev_alloc(&c.table, table_doubles, "class table") ||
        !dev_alloc(&c.flags, (size_t)npblk * S20_BS, "class flags") ||
        !dev_alloc(&c.counts, (size_t)npblk * S20_BS, "class scaler counts") ||
        !hip_ok(hipMemsetAsync(c.flags, 0, (size_t)npblk * S20_BS, e->stream), "memset flags"))
      return false;
    c.cap_classes = nclasses;
  }
  return true;
}

static unsigned long long class_child_version(const Engine * e, unsigned idx)
{
  return idx < e->tips ? e->tip_version[idx] : e->cherries[idx].version;
}

// the class table of a child was made under the code table in use (a tip's own classes do not depend on it)
static bool class_codes_match(const Engine * e, unsigned idx, unsigned lut_used)
{
  return idx < e->tips || e->cherries[idx].ncodes == lut_used;
}

// classes below a child of a class operation: a coded tip's codes, or the classes of a class node
static unsigned class_child_count(const Engine * e, unsigned idx, unsigned lut_used)
{
  return coded_tip(e, idx) ? lut_used : e->cherries[idx].nclasses;
}

// The class map of `node` as the parent of (c1, c2) -- both coded tips or class nodes with current maps -- :
// kept if it was made from these children, made on the device otherwise (one wait for the class count per new
// map of a node above cherries; a cherry needs none).  True if the node is worth keeping per class.
static bool class_map(Engine * e, unsigned node, unsigned c1, unsigned c2, unsigned lut_used, bool & failed)
{
  Engine::Cherry & c = e->cherries[node];
  failed = false;
  if (c.map_valid && c.ncodes == lut_used && c.child[0] == c1 && c.child[1] == c2 &&
      c.child_version[0] == class_child_version(e, c1) && c.child_version[1] == class_child_version(e, c2))
    return c.trackable;
  const unsigned n1 = class_child_count(e, c1, lut_used), n2 = class_child_count(e, c2, lut_used);
  const unsigned long long pairs = (unsigned long long)n1 * n2;
  c.map_valid = true;
  c.trackable = false;
  c.ncodes = lut_used;
  c.child[0] = c1; c.child[1] = c2;
  c.child_version[0] = class_child_version(e, c1); c.child_version[1] = class_child_version(e, c2);
  c.version = ++e->class_clock;
  e->plan.key.clear();
  if (!pairs) return false;
  failed = true;
  if (!c.pair && !dev_alloc(&c.pair, (size_t)e->Nalloc, "class codes")) return false;
  ClassMapArgs a;
  a.codes1 = coded_tip(e, c1) ? e->d_codes[c1] : nullptr;
  a.codes2 = coded_tip(e, c2) ? e->d_codes[c2] : nullptr;
  a.cls1 = coded_tip(e, c1) ? nullptr : e->cherries[c1].pair;
  a.cls2 = coded_tip(e, c2) ? nullptr : e->cherries[c2].pair;
  a.n1 = n1; a.n2 = n2;
  const dim3 gs(std::max(1u, std::min((e->Nalloc + 255u) / 256u, 8u * e->cu_count)));
  if (coded_tip(e, c1) && coded_tip(e, c2))
  {
    // a cherry: every code pair is a class
    hipLaunchKernelGGL(k_class_cherry, gs, dim3(256), 0, e->stream, a, e->Nalloc, c.pair);
    if (hipGetLastError() != hipSuccess) { set_error(PLL_ERROR_HIP_RUNTIME, "class map launch failed"); return false; }
    c.nclasses = (unsigned)pairs;
    (void)hipFree(c.rep); c.rep = nullptr; c.rep_cap = 0;
    c.trackable = true;
    failed = false;
    return true;
  }
  // the pairs that occur are numbered through a table of all pairs, or through a hash table of 2 N .. 4 N slots
  static const unsigned env_ratio = getenv("PLLHIP_CLASS_MIN_RATIO") ? (unsigned)std::max(1, atoi(getenv("PLLHIP_CLASS_MIN_RATIO"))) : 0u;
  const unsigned ratio = env_ratio ? env_ratio : (e->family == KernelFamily::S4 ? CLASS_MIN_RATIO_S4 : CLASS_MIN_RATIO_S20);
  const unsigned max_classes = (unsigned)std::min<unsigned long long>(pairs, e->N / ratio);
  // (PLLHIP_CLASS_TABLE_PAIRS: the largest table of possible pairs, for tests of the hash numbering on small inputs)
  static const unsigned long long env_pairs = getenv("PLLHIP_CLASS_TABLE_PAIRS") ? strtoull(getenv("PLLHIP_CLASS_TABLE_PAIRS"), nullptr, 10) : 0ULL;
  const bool hashed = pairs > (env_pairs ? std::min(env_pairs, CLASS_MAX_PAIRS) : CLASS_MAX_PAIRS);
  unsigned long long slots = pairs;
  if (hashed)
  {
    slots = 1024;
    while (slots < 2ULL * e->N) slots <<= 1;
    if (slots > CLASS_MAX_PAIRS) { failed = false; return false; }       // (alignments beyond 2 M sites: not numbered)
  }
  if (!max_classes) { failed = false; return false; }
  // scratch: seen[slots] | tile sums [1024] | total | (hashed) keys[slots], 8-byte aligned
  const size_t words = (size_t)slots + 1024 + 4 + (hashed ? 2 * (size_t)slots : 0);
  if (e->class_seen_cap < words)
  {
    if (hipStreamSynchronize(e->stream) != hipSuccess) return false;
    (void)hipFree(e->d_class_seen); e->d_class_seen = nullptr; e->class_seen_cap = 0;
    if (!dev_alloc(&e->d_class_seen, words, "class numbering scratch")) return false;
    e->class_seen_cap = words;
  }
  if (!e->h_class_total && !hip_ok(hipHostMalloc(reinterpret_cast<void **>(&e->h_class_total), sizeof(unsigned), hipHostMallocDefault), "hipHostMalloc"))
    return false;
  if (c.rep_cap < max_classes)
  {
    if (hipStreamSynchronize(e->stream) != hipSuccess) return false;
    (void)hipFree(c.rep); c.rep = nullptr; c.rep_cap = 0;
    if (!dev_alloc(&c.rep, 2 * (size_t)max_classes, "class children")) return false;
    c.rep_cap = max_classes;
  }
  unsigned * seen = e->d_class_seen, * tiles = seen + slots, * total = tiles + 1024;
  unsigned long long * keys = hashed ? reinterpret_cast<unsigned long long *>(seen + ((slots + 1024 + 2 + 1) & ~(size_t)1)) : nullptr;
  const unsigned ntiles = (unsigned)((slots + 4095) / 4096), mask = (unsigned)(slots - 1);
  if (!hip_ok(hipMemsetAsync(seen, 0, (size_t)slots * sizeof(unsigned), e->stream), "memset class scratch")) return false;
  if (hashed)
  {
    if (!hip_ok(hipMemsetAsync(keys, 0, (size_t)slots * sizeof(unsigned long long), e->stream), "memset class scratch")) return false;
    hipLaunchKernelGGL(k_class_hash_insert, gs, dim3(256), 0, e->stream, a, e->N, keys, seen, mask);
  }
  else hipLaunchKernelGGL(k_class_mark, gs, dim3(256), 0, e->stream, a, e->N, seen);
  hipLaunchKernelGGL(k_class_scan_tiles, dim3(ntiles), dim3(1024), 0, e->stream, seen, (unsigned)slots, tiles);
  hipLaunchKernelGGL(k_class_scan_top, dim3(1), dim3(1024), 0, e->stream, tiles, ntiles, total);
  hipLaunchKernelGGL(k_class_scan_apply, dim3(ntiles), dim3(1024), 0, e->stream, seen, (unsigned)slots, tiles, n2, c.rep, c.rep_cap,
                     (const unsigned long long *)keys);
  if (hipGetLastError() != hipSuccess) { set_error(PLL_ERROR_HIP_RUNTIME, "class map launch failed"); return false; }
  if (!hip_ok(hipMemcpyAsync(e->h_class_total, total, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream), "class count") ||
      !hip_ok(hipStreamSynchronize(e->stream), "class count")) return false;
  failed = false;
  c.nclasses = *e->h_class_total;
  if (!c.nclasses || c.nclasses > max_classes) return false;
  if (hashed) hipLaunchKernelGGL(k_class_hash_assign, gs, dim3(256), 0, e->stream, a, e->N, e->Nalloc, (const unsigned long long *)keys,
                                 (const unsigned *)seen, mask, c.pair);
  else hipLaunchKernelGGL(k_class_assign, gs, dim3(256), 0, e->stream, a, e->N, e->Nalloc, (const unsigned *)seen, c.pair);
  if (hipGetLastError() != hipSuccess) { set_error(PLL_ERROR_HIP_RUNTIME, "class map launch failed"); failed = true; return false; }
  c.trackable = true;
  return true;
}

// after the launches of a resident schedule: the operations whose vectors it left out (PlanOp::flags bit 0) go into
// the ledger, with the deferred runs of the schedule (kind: TRANSIENT_MODE / TRANSIENT_DEFERRED)
static void record_unstored(Engine * e, const pll_operation_t * ops, unsigned count, const DevicePlan & dp, char kind)
{
  const PlanOp * pops = reinterpret_cast<const PlanOp *>(dp.bytes.data());
  std::vector<unsigned> left_out;
  for (unsigned i = 0; i < dp.nops; ++i)
    if (pops[i].flags & 1u) left_out.push_back(pops[i].d.parent_index);
  e->ledger.after_list(ops, count, left_out, dp.defer_runs, kind);
}

// resolve one operation to device pointers and add its algorithmic bytes
// (child vectors in -- 8*S per (site, rate), a coded tip is 1 byte
// per site --, parent vector out, scalers, the two P-matrices or lookup tables
// once per op) and flops (a 2*S*S matvec per non-tip child + S products)
static void fill_desc(const Engine * e, const pll_operation_t & op, OpDesc & d, double & bytes, double & flops)
{
  const size_t pm_stride = (size_t)e->R * e->S * e->Sp;
  const size_t lut_stride = (size_t)e->R * e->lut_codes * e->S;
  const bool t1 = tip_coded(e, op.child1_clv_index);
  const bool t2 = tip_coded(e, op.child2_clv_index);
  d.clv1 = t1 ? nullptr : e->d_clv[op.child1_clv_index];
  d.codes1 = t1 ? e->d_codes[op.child1_clv_index] : nullptr;
  d.pmat1 = e->d_pmat + pm_stride * op.child1_matrix_index;
  d.pfrag1 = e->d_pfrag ? e->d_pfrag + (size_t)op.child1_matrix_index * e->R * 400 : nullptr;
  d.pfrag2 = e->d_pfrag ? e->d_pfrag + (size_t)op.child2_matrix_index * e->R * 400 : nullptr;
  d.lut1 = t1 ? e->d_lut + lut_stride * op.child1_matrix_index : nullptr;
  d.clv2 = t2 ? nullptr : e->d_clv[op.child2_clv_index];
  d.codes2 = t2 ? e->d_codes[op.child2_clv_index] : nullptr;
  d.pmat2 = e->d_pmat + pm_stride * op.child2_matrix_index;
  d.lut2 = t2 ? e->d_lut + lut_stride * op.child2_matrix_index : nullptr;
  d.scaler1 = scaler_ptr(e, op.child1_scaler_index);
  d.scaler2 = scaler_ptr(e, op.child2_scaler_index);
  d.parent = e->d_clv[op.parent_clv_index];
  d.parent_index = op.parent_clv_index;
  d.child1_index = op.child1_clv_index;
  d.child2_index = op.child2_clv_index;
  d.parent_scaler = const_cast<unsigned *>(scaler_ptr(e, op.parent_scaler_index));
  const double nr = (double)e->N * e->R;
  bytes += nr * 8.0 * e->S * (1.0 + (t1 ? 0.0 : 1.0) + (t2 ? 0.0 : 1.0));
  bytes += (double)e->N * ((t1 ? 1.0 : 0.0) + (t2 ? 1.0 : 0.0));
  bytes += (double)e->N * 4.0 * ((d.scaler1 ? 1 : 0) + (d.scaler2 ? 1 : 0) + (d.parent_scaler ? 1 : 0));
  bytes += 8.0 * e->R * e->S * ((t1 ? (double)e->lut_codes : (double)e->Sp) +
                                (t2 ? (double)e->lut_codes : (double)e->Sp));
  flops += nr * (2.0 * e->S * e->S * ((t1 ? 0.0 : 1.0) + (t2 ? 0.0 : 1.0)) + e->S);
}

// The device-resident schedule of an operation list (chains in dependency order, DevicePlan) in e->plan:
// built unless the cached one was made from the same list and settings.  mode 1: the whole traversal in
// one launch (chains depth first); mode 0: one launch per round of chains.  false: the list does not have
// the shape of a tree traversal (analyse_list, chain_plan.hpp).
static std::atomic<unsigned long long> plan_generation{0};

struct ScheduleRequest
{
  const pll_operation_t * ops;                   // the list as the caller passed it
  unsigned count;
  unsigned mode;
  bool transient;                                // an evaluate-only traversal (pllhip_set_transient)
  const RepeatPlan * rp;                         // site repeats: the class operations and the rest (null: none)
  bool fold = false;                             // lone cherries may be folded into the chains that read them (plan_folds)
};

struct ScheduleBuild                             // the schedule being built (DevicePlan::bytes)
{
  std::vector<PlanOp> pops;
  std::vector<PlanChain> pchains;
  std::vector<PairLutJob> pair_jobs;             // row tables of the wide tips of the chains
  std::vector<CherryJob> cherry_jobs;            // class operations, by level
  std::vector<PairLutJob> level_pairs;           // row tables of class children, by level of their parent
  size_t pairlut_used = 0;                       // doubles of e->d_pairlut handed out
  unsigned nops = 0, lds_max = 0;
  unsigned nfolds = 0, inner_reads = 0;          // folded cherries; inner vectors that the chains read from memory
  unsigned nlookups = 0;                         // children read through their class tables
  unsigned ndeferred = 0;                        // stores left out of a storing traversal
};

// site repeats: children that are cherries kept per class are read as wide tips (kernels_repeats.hpp);
// wide[2 k + x] for child x of operation k
static bool mark_wide_tips(Engine * e, const pll_operation_t * ops, unsigned count, unsigned lut_used,
                           std::vector<unsigned char> & wide, unsigned & nwide)
{
  wide.assign(e->cherries.empty() ? 0 : 2 * (size_t)count, 0);
  nwide = 0;
  if (wide.empty()) return true;
  std::vector<char> made(e->nodes, 0);
  for (unsigned k = 0; k < count; ++k)
  {
    const unsigned child[2] = {ops[k].child1_clv_index, ops[k].child2_clv_index};
    const int child_scaler[2] = {ops[k].child1_scaler_index, ops[k].child2_scaler_index};
    for (int x = 0; x < 2; ++x)
    {
      // (counts of a buffer that another class node stands for: written out first)
      if (child_scaler[x] >= 0 && e->scaler_lazy[child_scaler[x]] >= 0 && e->scaler_lazy[child_scaler[x]] != (int)child[x] &&
          !need_scaler(e, child_scaler[x])) return false;
      if (coded_tip(e, child[x]) || made[child[x]] || !e->cherries[child[x]].valid) continue;
      // (a cherry built under another code table -- a tip has taken a new ambiguity code since -- is read
      // through its expanded vector: its classes are not the ones this schedule indexes; so is a class node whose
      // counts are asked for under another scale buffer than the one its operation wrote)
      const Engine::Cherry & cc = e->cherries[child[x]];
      if (class_codes_match(e, child[x], lut_used) && (child_scaler[x] == cc.scaler_index)) { wide[2 * k + x] = 1; ++nwide; }
      else if (!need_clv(e, child[x])) return false;
    }
    made[ops[k].parent_clv_index] = 1;
  }
  return true;
}

// the cache key: the list as the caller passed it (the cherries taken out of it are part of the schedule), the codes
// in use, the mode, the wide tips, and which operations are kept per class (the same list can meet other class nodes
// of earlier calls)
static std::vector<unsigned char> schedule_key(const ScheduleRequest & rq, unsigned lut_used, const std::vector<unsigned char> & wide,
                                               bool fold, unsigned look_classes, DeferPolicy defer)
{
  std::vector<unsigned char> tracked(rq.rp ? rq.count : 0, 0);
  if (rq.rp) for (unsigned k : rq.rp->cherry_ops) tracked[k] = 1;
  const size_t list_bytes = (size_t)rq.count * sizeof(pll_operation_t);
  const unsigned mode_key = rq.mode | (rq.transient ? 0x100u : 0u) | (fold ? 0x200u : 0u);
  // (look_classes: the class limit of plan_lookups; defer: the policy of plan_defers)
  const unsigned head[] = {rq.count, lut_used, mode_key, look_classes, defer.level, defer.depth};
  std::vector<unsigned char> key(sizeof(head) + list_bytes + wide.size() + tracked.size());
  memcpy(key.data(), head, sizeof(head));
  memcpy(key.data() + sizeof(head), rq.ops, list_bytes);
  if (!wide.empty()) memcpy(key.data() + sizeof(head) + list_bytes, wide.data(), wide.size());
  if (!tracked.empty()) memcpy(key.data() + key.size() - tracked.size(), tracked.data(), tracked.size());
  return key;
}

// room in e->d_pairlut for the row tables of the schedule: one per (class node, branch above it) -- the wide tips of
// the chains and the class children of the class operations
static bool reserve_pair_tables(Engine * e, const ScheduleRequest & rq, const pll_operation_t * ops, unsigned count,
                                const std::vector<unsigned char> & wide)
{
  size_t rows = 0;
  for (unsigned k = 0; k < count && !wide.empty(); ++k)
  {
    if (wide[2 * k]) rows += e->cherries[ops[k].child1_clv_index].nclasses;
    if (wide[2 * k + 1]) rows += e->cherries[ops[k].child2_clv_index].nclasses;
  }
  if (rq.rp)
    for (unsigned k : rq.rp->cherry_ops)
    {
      if (!coded_tip(e, rq.ops[k].child1_clv_index)) rows += e->cherries[rq.ops[k].child1_clv_index].nclasses;
      if (!coded_tip(e, rq.ops[k].child2_clv_index)) rows += e->cherries[rq.ops[k].child2_clv_index].nclasses;
    }
  const size_t need = rows * e->R * e->S;
  if (need <= e->pairlut_cap) return true;
  if (hipStreamSynchronize(e->stream) != hipSuccess) return false;
  (void)hipFree(e->d_pairlut);
  e->d_pairlut = nullptr;
  e->pairlut_cap = 0;
  if (!dev_alloc(&e->d_pairlut, 2 * need, "wide-tip lookup tables")) return false;
  e->pairlut_cap = 2 * need;
  return true;
}

// room in e->d_looktab for the tables of the children read by tip codes (plan_lookups): per child, and per cherry below
// a cherry x tip child, the class table (blocked like a vector over the classes), its scaling flags and scaler counts
// per class, and its rows through the branch above it.  Allocated here, with the schedule: a traversal allocates nothing
// room: per entry of plan.lookups, where its tables are
static bool reserve_lookup_tables(Engine * e, const ChainPlan & plan, unsigned lut_used, std::vector<LookupRoom> & room)
{
  room.assign(plan.lookups.size(), LookupRoom());
  if (plan.lookups.empty()) return true;
  size_t need = 0;
  auto take = [&](size_t bytes) { const size_t at = need; need += (bytes + 255) & ~(size_t)255; return at; };
  for (size_t i = 0; i < plan.lookups.size(); ++i)
    for (int x = 0; x < (plan.lookups[i].cherry >= 0 ? 2 : 1); ++x)
    {
      const size_t classes = x ? (size_t)lut_used * lut_used : plan.lookups[i].nclasses, npblk = (classes + S20_BS - 1) / S20_BS;
      room[i].off_table[x] = take(npblk * e->R * S20_UNIT * sizeof(double));
      room[i].off_flags[x] = take(npblk * S20_BS);
      room[i].off_counts[x] = take(npblk * S20_BS * sizeof(unsigned));
      room[i].off_rows[x] = take(classes * e->R * e->S * sizeof(double));
    }
  if (need <= e->looktab_cap) return true;
  if (hipStreamSynchronize(e->stream) != hipSuccess) return false;      // a running traversal may still read the old tables
  (void)hipFree(e->d_looktab);
  e->d_looktab = nullptr;
  e->looktab_cap = 0;
  if (!dev_alloc(&e->d_looktab, need, "class tables of looked-up children")) return false;
  e->looktab_cap = need;
  return true;
}

// the row table of class node `c` through matrix `matrix` (the branch above it): its job, and where it will be
static const double * push_pair_job(const Engine * e, const ChainFamily & f, const Engine::Cherry & c, unsigned matrix,
                                    ScheduleBuild & sb, std::vector<PairLutJob> & jobs)
{
  PairLutJob job;
  job.table = c.table;
  job.pfrag = f.pair_pfrag(e, matrix);
  job.out = e->d_pairlut + sb.pairlut_used;
  job.nrows = c.nclasses;
  sb.pairlut_used += (size_t)e->R * c.nclasses * e->S;
  jobs.push_back(job);
  return job.out;
}

// the last launch of the schedule ends here: its running totals become its own share
static void close_launch(DevicePlan & dp, const ScheduleBuild & sb)
{
  if (dp.launches.empty()) return;
  DevicePlan::Launch & done = dp.launches.back();
  done.end = (unsigned)sb.pchains.size();
  done.ops = sb.nops - done.ops;
  done.bytes = dp.algo_bytes - done.bytes; done.flops = dp.algo_flops - done.flops; done.min_bytes = dp.min_bytes - done.min_bytes;
}

// the PlanOp / PlanChain entries of the chains in `order`, and the launches they fall into (the last one left open)
static void emit_chains(const Engine * e, const ChainFamily & f, const pll_operation_t * ops, const ChainPlan & plan,
                        const std::vector<size_t> & order, const std::vector<unsigned char> & wide, unsigned lut_used,
                        const ScheduleRequest & rq, DevicePlan & dp, ScheduleBuild & sb)
{
  const bool by_rounds = rq.mode == 0;
  dp.algo_bytes = dp.algo_flops = dp.min_bytes = 0.0;
  dp.launches.clear();
  int cur_round = -1;
  const unsigned chain_flags = f.tables_in_lds(e, lut_used) ? 1u : 0u;
  for (size_t c : order)
  {
    const std::vector<unsigned> & ch = plan.chains[c];
    if (dp.launches.empty() || (by_rounds && plan.launch[c] != cur_round))
    {
      close_launch(dp, sb);
      const unsigned at = (unsigned)sb.pchains.size();     // (ops, bytes, ...: running totals until the launch is closed)
      dp.launches.push_back({at, at, 1, sb.nops, dp.algo_bytes, dp.algo_flops, dp.min_bytes});
      cur_round = plan.launch[c];
    }
    sb.pchains.push_back({sb.nops, (unsigned)ch.size(), f.extent(e), e->lut_codes, lut_used, chain_flags});
    unsigned off = 0;
    unsigned fold_side = 0;                       // the operation in front is a cherry folded into this one (as child 1 / 2)
    bool first = true;                            // the first operation of the chain that is not folded
    for (size_t i = 0; i < ch.size(); ++i)
    {
      pll_operation_t o = ops[ch[i]];
      PlanOp & po = sb.pops[sb.nops++];
      memset(&po, 0, sizeof(po));
      const double before = dp.algo_bytes;
      const unsigned folded = plan.folded.empty() ? 0u : plan.folded[ch[i]];
      const unsigned looked = plan.looked.empty() ? 0u : plan.looked[ch[i]];
      po.carried = first ? 0 : plan.carried[ch[i]];
      if (!folded) first = false;
      if (fold_side == 1 || looked == 1)          // the folded cherry / the child read by tip codes is child 2 (products commute)
      {
        std::swap(o.child1_clv_index, o.child2_clv_index);
        std::swap(o.child1_matrix_index, o.child2_matrix_index);
        std::swap(o.child1_scaler_index, o.child2_scaler_index);
        if (po.carried) po.carried = 3 - po.carried;
        if (fold_side) fold_side = 2;
      }
      fill_desc(e, o, po.d, dp.algo_bytes, dp.algo_flops);
      // an evaluate-only traversal: the vectors inside a chain are handed on in registers only
      po.flags = (rq.transient && i + 1 < ch.size()) ? 1u : 0u;
      // a storing traversal: the stores nobody reads are left for later (plan_defers)
      if (!plan.deferred.empty() && plan.deferred[ch[i]]) { po.flags |= 1u; ++sb.ndeferred; }
      if (folded)
      {
        // a folded cherry: bit 3 here, bit 4 on its consumer (the next entry); its two tip tables and, behind
        // them, its scaling decisions per pair of codes take fold_lds doubles of the chain's LDS
        po.flags |= 8u;
        sb.pchains.back().flags |= 2u;
        ++sb.nfolds;
        dp.min_bytes += dp.algo_bytes - before - ((po.flags & 1u) ? (double)e->N * e->R * 8.0 * e->S : 0.0);
        po.slot1 = off;
        po.slot2 = off + child_table_lds(e, f, o.child1_clv_index, lut_used, false);
        off += f.fold_lds(e, lut_used);
        fold_side = folded;
        continue;
      }
      if (fold_side) po.flags |= 16u;
      for (unsigned x = 1; x <= 2; ++x)
      {
        const unsigned idx = x == 1 ? o.child1_clv_index : o.child2_clv_index;
        const bool w_x = !wide.empty() && wide[2 * ch[i] + x - 1];
        if (idx >= e->tips && !w_x && po.carried != x && fold_side != x && !(looked && x == 2)) ++sb.inner_reads;
      }
      double wide_saved = (po.flags & 1u) ? (double)e->N * e->R * 8.0 * e->S : 0.0;
      const bool w[2] = {!wide.empty() && wide[2 * ch[i]], !wide.empty() && wide[2 * ch[i] + 1]};
      for (int x = 0; x < 2; ++x)
      {
        if (!w[x]) continue;
        const Engine::Cherry & cc = e->cherries[x ? o.child2_clv_index : o.child1_clv_index];
        const double * rows = push_pair_job(e, f, cc, x ? o.child2_matrix_index : o.child1_matrix_index, sb, sb.pair_jobs);
        // wide tip: no vector, no byte codes; pfrag = class codes, lut = its table, childN_index = table rows
        // (... and its scaler counts per class)
        // (bit 1 / 2 of the flags: few rows, staged in LDS by the chain kernels of the 20- and 2 .. 32-state families)
        if (f.wide_lds(e, cc.nclasses)) po.flags |= 2u << x;
        if (x) { po.d.clv2 = nullptr; po.d.codes2 = nullptr; po.d.pfrag2 = reinterpret_cast<const double *>(cc.pair); po.d.lut2 = rows; po.d.child2_index = cc.nclasses;
                 if (po.d.scaler2) po.d.scaler2 = cc.counts; }
        else   { po.d.clv1 = nullptr; po.d.codes1 = nullptr; po.d.pfrag1 = reinterpret_cast<const double *>(cc.pair); po.d.lut1 = rows; po.d.child1_index = cc.nclasses;
                 if (po.d.scaler1) po.d.scaler1 = cc.counts; }
        wide_saved += (double)e->N * e->R * 8.0 * e->S - 4.0 * e->N;      // class codes instead of the vector
      }
      // the handed-over child stays in registers: neither its vector nor its scaler counts are read
      dp.min_bytes += dp.algo_bytes - before - wide_saved;
      if (po.carried)
        dp.min_bytes -= (double)e->N * e->R * 8.0 * e->S +
                        ((po.carried == 1 ? po.d.scaler1 : po.d.scaler2) ? 4.0 * (double)e->N * (e->rate_scalers ? e->R : 1) : 0.0);
      // ... and so does a folded cherry
      if (fold_side)
        dp.min_bytes -= (double)e->N * e->R * 8.0 * e->S + ((fold_side == 1 ? po.d.scaler1 : po.d.scaler2) ? 4.0 * (double)e->N : 0.0);
      fold_side = 0;
      // ... and a child read through its class table: two or three code bytes per site instead of vector and counts
      // (emit_lookup_tables completes the entry)
      if (looked)
      {
        po.flags |= 32u;
        ++sb.nlookups;
        dp.min_bytes -= (double)e->N * e->R * 8.0 * e->S + (po.d.scaler2 ? 4.0 * (double)e->N : 0.0);
      }
      po.slot1 = off;
      off += child_table_lds(e, f, o.child1_clv_index, lut_used, w[0]);
      po.slot2 = off;
      off += child_table_lds(e, f, o.child2_clv_index, lut_used, w[1]);
    }
    sb.lds_max = std::max(sb.lds_max, f.lds_is_length ? (unsigned)ch.size() : off);
  }
}

// site repeats: the operations the schedule keeps per class (taken out of the list by the caller), by level, with the
// row tables of their class children
static void emit_repeat_levels(const Engine * e, const ChainFamily & f, const ScheduleRequest & rq, DevicePlan & dp,
                               ScheduleBuild & sb)
{
  dp.repeat_levels.clear();
  dp.repeat_classes = 0;
  if (!rq.rp) return;
  const size_t lut_stride = (size_t)e->R * e->lut_codes * e->S;
  const size_t nrp = rq.rp->cherry_ops.size();
  std::vector<int> node_level(e->nodes, -1);
  std::vector<unsigned> lvl(nrp, 0), order(nrp);
  unsigned max_level = 0;
  for (size_t x = 0; x < nrp; ++x)
  {
    const pll_operation_t & o = rq.ops[rq.rp->cherry_ops[x]];
    unsigned l = 0;
    if (o.child1_clv_index >= e->tips) l = std::max(l, 1u + (unsigned)std::max(node_level[o.child1_clv_index], 0));
    if (o.child2_clv_index >= e->tips) l = std::max(l, 1u + (unsigned)std::max(node_level[o.child2_clv_index], 0));
    lvl[x] = l;
    node_level[o.parent_clv_index] = (int)l;
    max_level = std::max(max_level, l);
    order[x] = (unsigned)x;
  }
  std::stable_sort(order.begin(), order.end(), [&](unsigned a, unsigned b) { return lvl[a] < lvl[b]; });
  size_t at = 0;
  for (unsigned l = 0; l <= max_level; ++l)
  {
    DevicePlan::RepeatLevel L = {(unsigned)sb.cherry_jobs.size(), 0, (unsigned)sb.level_pairs.size(), 0, 0, 0};
    for (; at < nrp && lvl[order[at]] == l; ++at)
    {
      const pll_operation_t & o = rq.ops[rq.rp->cherry_ops[order[at]]];
      const Engine::Cherry & c = e->cherries[o.parent_clv_index];
      CherryJob j;
      memset(&j, 0, sizeof(j));
      const unsigned child[2] = {o.child1_clv_index, o.child2_clv_index};
      const unsigned matrix[2] = {o.child1_matrix_index, o.child2_matrix_index};
      const int child_scaler[2] = {o.child1_scaler_index, o.child2_scaler_index};
      for (int x = 0; x < 2; ++x)
      {
        const double * rows;
        unsigned nrows;
        if (coded_tip(e, child[x])) { rows = e->d_lut + lut_stride * matrix[x]; nrows = e->lut_codes; }
        else
        {
          const Engine::Cherry & cc = e->cherries[child[x]];
          rows = push_pair_job(e, f, cc, matrix[x], sb, sb.level_pairs);
          nrows = cc.nclasses;
          L.max_rows = std::max(L.max_rows, cc.nclasses);
        }
        const unsigned * cnt = (child[x] >= e->tips && child_scaler[x] >= 0) ? e->cherries[child[x]].counts : nullptr;
        if (x) { j.lut2 = rows; j.rows2 = nrows; j.cnt2 = cnt; }
        else   { j.lut1 = rows; j.rows1 = nrows; j.cnt1 = cnt; }
      }
      j.rep = c.rep;
      j.nclasses = c.nclasses;
      j.table = c.table; j.flags = c.flags;
      j.counts = o.parent_scaler_index >= 0 ? c.counts : nullptr;
      sb.cherry_jobs.push_back(j);
      L.max_classes = std::max(L.max_classes, c.nclasses);
      dp.repeat_classes += c.nclasses;
      // what SURVEY.md 8d counts for the operation / what it moves now
      OpDesc dummy;
      double ab = 0.0;
      fill_desc(e, o, dummy, ab, dp.algo_flops);
      dp.algo_bytes += ab;
      dp.min_bytes += 2.0 * e->N + 4.0 * e->N;            // (tip codes in once per topology; a class code per site for the consumer)
    }
    L.job_end = (unsigned)sb.cherry_jobs.size();
    L.pair_end = (unsigned)sb.level_pairs.size();
    dp.repeat_levels.push_back(L);
  }
}

// The tables of the children read by tip codes (plan_lookups), dense over all U^2 / U^3 tuples of codes, through the
// class kernels of site repeats (kernels_repeats.hpp) -- whose consumers are pinned to give, bit for bit, what they
// compute from the stored vector -- in two levels that all such children of the schedule share:
//   the cherries' tables (class = code1 * U + code2: the kernel's own arithmetic, no class map);
//   their rows through the branch above each, then the tables of the cherry x tip operations from those rows and
//   the tip's (class = cherry class * U + tip code: the same arithmetic with U^2 rows on one side), with the scaling
//   decision and the summed counts per class;
//   the rows of those through the branch above them (pack_schedule's last level).
// The consumers' entries get the tip code arrays, the rows and the counts (PlanOp::flags bit 5).
static void emit_lookup_tables(const Engine * e, const ChainFamily & f, const pll_operation_t * ops, const ChainPlan & plan,
                               const std::vector<LookupRoom> & room, unsigned lut_used, DevicePlan & dp, ScheduleBuild & sb)
{
  if (plan.lookups.empty()) return;
  const size_t lut_stride = (size_t)e->R * e->lut_codes * e->S;
  const unsigned pairs = lut_used * lut_used;
  std::vector<int> entry_of(e->nodes, -1);
  for (unsigned i = 0; i < sb.nops; ++i) entry_of[sb.pops[i].d.parent_index] = (int)i;
  auto room_of = [&](const ChainPlan::Lookup & l) -> const LookupRoom & { return room[&l - plan.lookups.data()]; };
  auto table = [&](const ChainPlan::Lookup & l, int x) { return reinterpret_cast<double *>(e->d_looktab + room_of(l).off_table[x]); };
  auto counts = [&](const ChainPlan::Lookup & l, int x) { return reinterpret_cast<unsigned *>(e->d_looktab + room_of(l).off_counts[x]); };
  auto rows = [&](const ChainPlan::Lookup & l, int x) { return reinterpret_cast<double *>(e->d_looktab + room_of(l).off_rows[x]); };
  // the matrix of the branch above `child` in operation o
  auto matrix_above = [&](const pll_operation_t & o, unsigned child)
  { return o.child1_clv_index == child ? o.child1_matrix_index : o.child2_matrix_index; };
  DevicePlan::RepeatLevel L0 = {(unsigned)sb.cherry_jobs.size(), 0, (unsigned)sb.level_pairs.size(), (unsigned)sb.level_pairs.size(), pairs, 0};
  for (const ChainPlan::Lookup & l : plan.lookups)
  {
    const int x = l.cherry >= 0 ? 1 : 0;
    const pll_operation_t & c = ops[x ? (unsigned)l.cherry : l.top];
    CherryJob j;
    memset(&j, 0, sizeof(j));
    j.lut1 = e->d_lut + lut_stride * c.child1_matrix_index; j.rows1 = e->lut_codes;
    j.lut2 = e->d_lut + lut_stride * c.child2_matrix_index; j.rows2 = e->lut_codes;
    j.nclasses = pairs;
    j.table = table(l, x);
    j.flags = e->d_looktab + room_of(l).off_flags[x];
    j.counts = c.parent_scaler_index >= 0 ? counts(l, x) : nullptr;
    sb.cherry_jobs.push_back(j);
  }
  L0.job_end = (unsigned)sb.cherry_jobs.size();
  dp.repeat_levels.push_back(L0);
  DevicePlan::RepeatLevel L1 = {L0.job_end, 0, L0.pair_end, 0, 0, pairs};
  for (const ChainPlan::Lookup & l : plan.lookups)
  {
    const pll_operation_t & t = ops[l.top], & k = ops[l.consumer];
    const int x = l.cherry >= 0 ? 1 : 0;
    const pll_operation_t & c = ops[x ? (unsigned)l.cherry : l.top];
    // the cherry's rows through the branch above it: into the cherry x tip operation, or into the consumer
    PairLutJob pj;
    pj.table = table(l, x);
    pj.pfrag = f.pair_pfrag(e, matrix_above(x ? t : k, c.parent_clv_index));
    pj.out = rows(l, x);
    pj.nrows = pairs;
    sb.level_pairs.push_back(pj);
    if (!x) continue;
    const bool cherry_first = t.child1_clv_index == c.parent_clv_index;
    const unsigned tip = cherry_first ? t.child2_clv_index : t.child1_clv_index;
    CherryJob j;
    memset(&j, 0, sizeof(j));
    j.lut1 = rows(l, 1); j.rows1 = pairs;
    j.lut2 = e->d_lut + lut_stride * matrix_above(t, tip); j.rows2 = e->lut_codes;
    j.cnt1 = (cherry_first ? t.child1_scaler_index : t.child2_scaler_index) >= 0 ? counts(l, 1) : nullptr;
    j.nclasses = l.nclasses;
    j.table = table(l, 0);
    j.flags = e->d_looktab + room_of(l).off_flags[0];
    j.counts = t.parent_scaler_index >= 0 ? counts(l, 0) : nullptr;
    sb.cherry_jobs.push_back(j);
    L1.max_classes = std::max(L1.max_classes, l.nclasses);
    PairLutJob top;
    top.table = table(l, 0);
    top.pfrag = f.pair_pfrag(e, matrix_above(k, t.parent_clv_index));
    top.out = rows(l, 0);
    top.nrows = l.nclasses;
    sb.pair_jobs.push_back(top);
  }
  L1.job_end = (unsigned)sb.cherry_jobs.size();
  L1.pair_end = (unsigned)sb.level_pairs.size();
  dp.repeat_levels.push_back(L1);
  // the consumers' entries (the child is child 2 there: emit_chains)
  for (const ChainPlan::Lookup & l : plan.lookups)
  {
    const pll_operation_t & t = ops[l.top];
    PlanOp & po = sb.pops[entry_of[ops[l.consumer].parent_clv_index]];
    unsigned tips[3] = {t.child1_clv_index, t.child2_clv_index, ~0u};
    if (l.cherry >= 0)
    {
      const pll_operation_t & c = ops[l.cherry];
      tips[2] = t.child1_clv_index == c.parent_clv_index ? t.child2_clv_index : t.child1_clv_index;
      tips[0] = c.child1_clv_index; tips[1] = c.child2_clv_index;
    }
    po.d.clv2 = reinterpret_cast<const double *>(e->d_codes[tips[0]]);
    po.d.pmat2 = reinterpret_cast<const double *>(e->d_codes[tips[1]]);
    po.d.pfrag2 = l.cherry >= 0 ? reinterpret_cast<const double *>(e->d_codes[tips[2]]) : nullptr;
    po.d.codes2 = nullptr;
    po.d.lut2 = rows(l, 0);
    po.d.child2_index = l.nclasses;
    if (po.d.scaler2) po.d.scaler2 = counts(l, 0);
    dp.min_bytes += (double)e->N * (l.cherry >= 0 ? 3.0 : 2.0);
  }
}

// DevicePlan::bytes: [PlanOp][PlanChain][CherryJob][PairLutJob]; the row tables of the wide tips of the chains go after
// the last level of class operations
static void pack_schedule(DevicePlan & dp, ScheduleBuild & sb, unsigned lut_used)
{
  if (!sb.cherry_jobs.empty() || !sb.pair_jobs.empty())
  {
    DevicePlan::RepeatLevel L = {(unsigned)sb.cherry_jobs.size(), (unsigned)sb.cherry_jobs.size(), (unsigned)sb.level_pairs.size(),
                                 (unsigned)(sb.level_pairs.size() + sb.pair_jobs.size()), 0, 0};
    for (const PairLutJob & pj : sb.pair_jobs) L.max_rows = std::max(L.max_rows, pj.nrows);
    dp.repeat_levels.push_back(L);
    sb.level_pairs.insert(sb.level_pairs.end(), sb.pair_jobs.begin(), sb.pair_jobs.end());
  }
  const std::vector<PairLutJob> & pairs = sb.level_pairs;
  dp.ncherry_jobs = (unsigned)sb.cherry_jobs.size();
  dp.npair_jobs = (unsigned)pairs.size();
  dp.repeat_codes = lut_used;
  dp.off_cherry_jobs = sb.pops.size() * sizeof(PlanOp) + sb.pchains.size() * sizeof(PlanChain);
  dp.off_pair_jobs = dp.off_cherry_jobs + sb.cherry_jobs.size() * sizeof(CherryJob);
  dp.bytes.resize(dp.off_pair_jobs + pairs.size() * sizeof(PairLutJob));
  memcpy(dp.bytes.data(), sb.pops.data(), sb.pops.size() * sizeof(PlanOp));
  memcpy(dp.bytes.data() + sb.pops.size() * sizeof(PlanOp), sb.pchains.data(), sb.pchains.size() * sizeof(PlanChain));
  if (!sb.cherry_jobs.empty()) memcpy(dp.bytes.data() + dp.off_cherry_jobs, sb.cherry_jobs.data(), sb.cherry_jobs.size() * sizeof(CherryJob));
  if (!pairs.empty()) memcpy(dp.bytes.data() + dp.off_pair_jobs, pairs.data(), pairs.size() * sizeof(PairLutJob));
}

// rounds of ONE chain each that follow one another (the spine towards the root) need no launch boundary between
// them: one workgroup row walks them in turn, exactly as in a one-launch traversal
static void merge_single_chain_rounds(DevicePlan & dp)
{
  std::vector<DevicePlan::Launch> merged;
  for (const DevicePlan::Launch & l : dp.launches)
  {
    if (!merged.empty() && l.end - l.begin == 1 && merged.back().rows == 1)
    {
      DevicePlan::Launch & m = merged.back();
      m.end = l.end;
      m.ops += l.ops; m.bytes += l.bytes; m.flops += l.flops; m.min_bytes += l.min_bytes;
    }
    else
    {
      merged.push_back(l);
      merged.back().rows = l.end - l.begin;
    }
  }
  dp.launches.swap(merged);
}

static bool prepare_schedule(Engine * e, const pll_partition_t * p, const ChainFamily & f, const ScheduleRequest & rq)
{
  const unsigned lut_used = std::max(1u, std::min(codes_in_use(e, p), e->lut_codes));
  const pll_operation_t * ops = rq.rp ? rq.rp->ops.data() : rq.ops;
  const unsigned count = rq.rp ? (unsigned)rq.rp->ops.size() : rq.count;
  DevicePlan & dp = e->plan;
  std::vector<unsigned char> wide;
  unsigned nwide = 0;
  if (!mark_wide_tips(e, ops, count, lut_used, wide, nwide)) return false;
  // (folds: not next to class nodes; PLLHIP_FOLD and the family decide the rest)
  const unsigned fold_lds = rq.fold && !rq.rp && !nwide ? fold_table_lds(e, f, lut_used) : 0u;
  // (children read through class tables: where folds are planned, in storing traversals)
  const unsigned look_classes = fold_lds && f.look_classes && !rq.transient && !e->transient_mode ? f.look_classes(e, lut_used) : 0u;
  // (deferred stores: where folds are planned, in storing traversals)
  const DeferPolicy defer = fold_lds ? defer_stores(e, f, rq.transient) : DeferPolicy();
  std::vector<unsigned char> key = schedule_key(rq, lut_used, wide, fold_lds != 0, look_classes, defer);
  if (!dp.key.empty() && dp.key == key) return true;
  if ((nwide || rq.rp) && !reserve_pair_tables(e, rq, ops, count, wide)) return false;
  const PlannedList pl(e, &f, ops, count, lut_used, &wide);
  if (!pl.accepted) return false;
  ChainPlan plan;
  plan_chains(pl.list, pl.facts, f.chain_max, f.chain_lds, plan);
  plan_folds(pl.list, pl.facts, f.chain_max, f.chain_lds, fold_lds, plan);
  plan_lookups(pl.facts, lut_used, look_classes, plan);
  if (defer.level) plan_defers(pl.facts, defer, plan);
  std::vector<LookupRoom> room;
  if (!reserve_lookup_tables(e, plan, lut_used, room)) return false;
  ScheduleBuild sb;
  sb.pops.resize(count);
  emit_chains(e, f, ops, plan, chain_order(pl.facts, plan, rq.mode == 0), wide, lut_used, rq, dp, sb);
  emit_repeat_levels(e, f, rq, dp, sb);
  emit_lookup_tables(e, f, ops, plan, room, lut_used, dp, sb);
  pack_schedule(dp, sb, lut_used);
  close_launch(dp, sb);                           // (the last launch also carries the class operations' bytes)
  if (rq.mode == 0) merge_single_chain_rounds(dp);
  else for (DevicePlan::Launch & l : dp.launches) l.rows = 1;
  dp.nops = sb.nops;
  dp.nchains = (unsigned)sb.pchains.size();
  dp.lds_doubles = sb.lds_max;
  dp.nfolds = sb.nfolds;
  dp.inner_reads = sb.inner_reads;
  dp.nlookups = sb.nlookups;
  dp.ndeferred = sb.ndeferred;
  dp.defer_runs.clear();
  for (unsigned k = 0; k < count && !plan.run_up.empty(); ++k)
    if (plan.run_up[k] >= 0) dp.defer_runs.emplace_back(ops[k].parent_clv_index, ops[plan.run_up[k]].parent_clv_index);
  dp.max_extent = f.extent(e);
  dp.generation = ++plan_generation;
  dp.key.swap(key);
  return true;
}

// the class operations and row tables of a resident schedule (kernels_repeats.hpp), on the engine's stream; the
// schedule's job arrays are on the device (upload_plan)
static int launch_class_levels(Engine * e, const ChainFamily & f, const DevicePlan & dp)
{
  // level by level: the row tables of the class children of a level, then the tables of the level (with the
  // scaler counts per class); the last entry holds the row tables of the wide tips of the chains
  const CherryJob * cj = reinterpret_cast<const CherryJob *>(dp.d_buf + dp.off_cherry_jobs);
  const PairLutJob * pj = reinterpret_cast<const PairLutJob *>(dp.d_buf + dp.off_pair_jobs);
  for (const DevicePlan::RepeatLevel & L : dp.repeat_levels)
  {
    if (L.pair_end > L.pair_begin)
    {
      f.pair_lut(e, pj + L.pair_begin, L.pair_end - L.pair_begin, L.max_rows);
      PLLHIP_TRY(hipGetLastError());
    }
    if (L.job_end > L.job_begin)
    {
      f.class_build(e, cj + L.job_begin, L.job_end - L.job_begin, L.max_classes, dp.repeat_codes);
      PLLHIP_TRY(hipGetLastError());
    }
  }
  return PLL_SUCCESS;
}

// index checks of an operation list (the reference interface returns nothing: errors go to pll_errno)
static int validate_ops(const Engine * e, const pll_operation_t * ops, unsigned count)
{
  for (unsigned k = 0; k < count; ++k)
  {
    const pll_operation_t & op = ops[k];
    if (!check_clv_index(e, op.parent_clv_index, "parent") ||
        !check_clv_index(e, op.child1_clv_index, "child1") ||
        !check_clv_index(e, op.child2_clv_index, "child2") ||
        !check_scaler_index(e, op.parent_scaler_index) ||
        !check_scaler_index(e, op.child1_scaler_index) ||
        !check_scaler_index(e, op.child2_scaler_index))
      return PLL_FAILURE;
    if (op.child1_matrix_index >= e->nmat || op.child2_matrix_index >= e->nmat)
    {
      set_error(PLL_ERROR_PARAM_INVALID, "matrix index out of range in operation %u", k);
      return PLL_FAILURE;
    }
    if (op.parent_clv_index < e->tips && e->coded_tips)
    {
      set_error(PLL_ERROR_PARAM_INVALID, "operation %u writes a coded tip", k);
      return PLL_FAILURE;
    }
  }
  return PLL_SUCCESS;
}

// profiling (pllhip_profile_*) and counting of one launch of the partials path: `launch` runs between the two events
// of a pair when profiling is on; bytes / flops / min_bytes / nops: what the launch stands for
template <class Launch>
static int counted_launch(Engine * e, double bytes, double flops, unsigned nops, double min_bytes, Launch && launch)
{
  hipEvent_t ev1 = nullptr;
  if (e->profiling)
  {
    if (e->prof_used == e->prof_events.size())
    {
      hipEvent_t x, y;
      PLLHIP_TRY(hipEventCreate(&x));
      PLLHIP_TRY(hipEventCreate(&y));
      e->prof_events.emplace_back(x, y);
    }
    ev1 = e->prof_events[e->prof_used].second;
    PLLHIP_TRY(hipEventRecord(e->prof_events[e->prof_used++].first, e->stream));
  }
  if (!launch()) return PLL_FAILURE;
  if (e->profiling)
  {
    PLLHIP_TRY(hipEventRecord(ev1, e->stream));
    e->prof_bytes += bytes;
    e->prof_min_bytes += min_bytes;
    e->prof_flops += flops;
    e->prof_ops += nops;
  }
  e->counters.partial_launches++;
  return PLL_SUCCESS;
}

static void count_list(Engine * e, unsigned count)
{
  e->counters.partial_ops += count;
  e->counters.site_updates += (unsigned long long)count * e->N * e->R;
}

// what comes before any schedule of a list: index checks, vectors of evaluate-only traversals, P-matrices and lookup
// tables, and the class nodes the list overwrites
static int begin_list(Engine * e, pll_partition_t * p, const pll_operation_t * ops, unsigned count)
{
  PLLHIP_TRY(hipSetDevice(e->device));
  if (!validate_ops(e, ops, count)) return PLL_FAILURE;
  // (before the queued P-matrices are launched: vectors that were not stored and that this list overwrites are given
  // up, the ones it reads are stored with the matrices they were made with; a list that stores such vectors --
  // transient_busy -- runs on the matrices the device holds)
  if (!e->ledger.empty())
  {
    std::vector<unsigned> want;
    std::vector<char> going;
    e->ledger.before_list(ops, count, e->nscalers, e->transient_busy, want, going);
    if (!want.empty() && !store_unstored(e, want, &going)) return PLL_FAILURE;
    e->ledger.give_up_written(ops, count, e->transient_busy);
  }
  if (e->shadow_codes)
    for (unsigned k = 0; k < count; ++k)
      if (ops[k].parent_clv_index < e->tips) e->tip_has_codes[ops[k].parent_clv_index] = 0;    // (a tip vector is overwritten)
  if ((!e->transient_busy && !flush_pmatrices(p)) || !ensure_luts(p)) return PLL_FAILURE;
  if (e->cherries.empty()) return PLL_SUCCESS;
  // every vector this list writes stops being the cherry it may have been; one that the list reads first
  // (and that exists per class only) is expanded before it goes
  // ... and the same for scale buffers whose counts exist per class only
  std::vector<char> read(e->nodes, 0), sread(e->nscalers, 0);
  for (unsigned k = 0; k < count; ++k)
  {
    read[ops[k].child1_clv_index] = read[ops[k].child2_clv_index] = 1;
    if (ops[k].child1_scaler_index >= 0) sread[ops[k].child1_scaler_index] = 1;
    if (ops[k].child2_scaler_index >= 0) sread[ops[k].child2_scaler_index] = 1;
    Engine::Cherry & c = e->cherries[ops[k].parent_clv_index];
    if (c.valid && read[ops[k].parent_clv_index] && !need_clv(e, ops[k].parent_clv_index)) return PLL_FAILURE;
    // the node stops being a class node: counts it stands for under a buffer this operation does not rewrite
    // are written out while its table still describes them
    if (c.valid && c.scaler_index >= 0 && e->scaler_lazy[c.scaler_index] == (int)ops[k].parent_clv_index &&
        c.scaler_index != ops[k].parent_scaler_index && !need_scaler(e, c.scaler_index)) return PLL_FAILURE;
    c.valid = false;
    const int sp = ops[k].parent_scaler_index;
    if (sp >= 0 && e->scaler_lazy[sp] >= 0)
    {
      if (sread[sp] && !need_scaler(e, sp)) return PLL_FAILURE;
      e->scaler_lazy[sp] = -1;
    }
  }
  return PLL_SUCCESS;
}

// the paths that read child scaler counts per site (everything but the resident schedules, whose wide tips read
// them per class): counts that exist per class only are written out first
static int plain_scalers(Engine * e, const pll_operation_t * ops, unsigned count)
{
  if (e->scaler_lazy.empty()) return PLL_SUCCESS;
  for (unsigned k = 0; k < count; ++k)
    if (!need_scaler(e, ops[k].child1_scaler_index) || !need_scaler(e, ops[k].child2_scaler_index)) return PLL_FAILURE;
  return PLL_SUCCESS;
}

// Device-resident schedules serve two forms: the whole traversal in one launch (1), or (lists of six operations and
// more) one launch per round with the chains of the round as grid rows (0); -1: neither.  In one launch a workgroup
// walks ALL chains one after the other and no launch boundary is paid; by rounds the chains run side by side (which
// is what a partition needs that does not fill the chip with its site blocks) and the workgroups of a round are
// shared out dynamically (which wins again on very large partitions).  Measured per traversal, rounds / one launch:
//   20 states, 200 taxa:  32 k sites 1.55 / 2.14 ms, 64 k 2.64 / 2.59, 125 k 4.83 / 4.66,
//                         250 k 8.66 / 8.93, 500 k 16.4 / 17.2, 1 M 32.4 / 33.0
//    4 states, 100 taxa:  100 k 0.52 / 0.58, 250 k 1.08 / 1.18, 500 k 1.94 / 1.99, 1 M 3.64 / 3.52
//   16 states,  50 taxa:  8 k 0.23 / 0.38, 32 k 0.36 / 0.44, 128 k 1.03 / 0.94, 500 k 3.22 / 3.17
//    2 states,  50 taxa:  1 M 2.20 / 2.74
// A repeated list is neither planned nor copied again (2.5 us of host time per launch), its kernels read their
// descriptors from device memory, a round is never split at 24 operations and rounds of single operations stay on
// the chain kernel: 72 -> 21 us and 212 -> 23 us per full-traversal call of a 2 000-site partition at 4 / 20 states
// against the by-value form (run_chains_by_value).  Short lists (the 1 - 3 operations of an SPR insertion) keep their
// descriptors in the kernel arguments: a schedule would have to be copied to the device first (W3 at C2 size: 165
// against 178 us per iteration) -- except in a family without the by-value form.
static int resident_mode(const Engine * e, const ChainFamily & f, unsigned count)
{
  // PLLHIP_TRAVERSE=1 / 0: whole traversals always / never in one launch (default: by size; never when several
  // partitions share the device, each on its own stream: long-lived workgroups with a fixed share of the sites
  // interleave worse than rounds -- two DNA + two protein partitions: 7.7 against 7.1 ms).
  static const int env_traverse = getenv("PLLHIP_TRAVERSE") ? atoi(getenv("PLLHIP_TRAVERSE")) : -1;
  const bool use_traverse = env_traverse >= 0 ? env_traverse != 0
                          : (engines_on_device[e->device & 63].load() <= 1 && f.fills_chip(e) && (count >= 6 || !f.chains));
  return use_traverse ? 1 : count >= 6 ? 0 : -1;
}

// site repeats: the cherries of the list that an operation of the list consumes are kept per class
// (kernels_repeats.hpp) and leave the list (rp.ops); their consumers read them as wide tips
static int select_class_ops(Engine * e, const pll_operation_t * ops, unsigned count, unsigned lut_used, RepeatPlan & rp)
{
  if (!e->site_repeats || lut_used > 64) return PLL_SUCCESS;
  // an operation is kept per class if an operation of the list consumes it and both children are known per
  // class: coded tips, class operations earlier in the list, or class nodes of earlier calls whose tables
  // still are their vectors
  std::vector<int> consumer(e->nodes, -1);
  std::vector<char> now(e->nodes, 0);
  for (unsigned k = 0; k < count; ++k) { consumer[ops[k].child1_clv_index] = (int)k; consumer[ops[k].child2_clv_index] = (int)k; }
  for (unsigned k = 0; k < count; ++k)
  {
    const pll_operation_t & o = ops[k];
    const unsigned child[2] = {o.child1_clv_index, o.child2_clv_index};
    const int child_scaler[2] = {o.child1_scaler_index, o.child2_scaler_index};
    bool ok = consumer[o.parent_clv_index] > (int)k && child[0] != child[1];
    for (int x = 0; x < 2 && ok; ++x)
    {
      if (coded_tip(e, child[x])) ok = child_scaler[x] == PLL_SCALE_BUFFER_NONE;
      else
      {
        const Engine::Cherry & cc = e->cherries[child[x]];
        ok = (now[child[x]] || cc.valid) && cc.map_valid && cc.trackable && class_codes_match(e, child[x], lut_used) &&
             child_scaler[x] == cc.scaler_index;          // (its counts per class are the ones asked for)
      }
    }
    if (ok)
    {
      bool failed = false;
      ok = class_map(e, o.parent_clv_index, child[0], child[1], lut_used, failed);
      if (failed) return PLL_FAILURE;
    }
    if (ok)
    {
      Engine::Cherry & c = e->cherries[o.parent_clv_index];
      if (!cherry_storage(e, o.parent_clv_index, c.nclasses)) return PLL_FAILURE;
      c.valid = true;
      c.materialized = false;
      c.scaler_index = o.parent_scaler_index;
      now[o.parent_clv_index] = 1;
      rp.cherry_ops.push_back(k);
    }
    else rp.ops.push_back(o);
  }
  if (!rp.cherry_ops.empty() && !rp.ops.empty())
  {
    rp.active = true;
    rp.ncodes = lut_used;
  }
  else
    for (unsigned k : rp.cherry_ops) e->cherries[ops[k].parent_clv_index].valid = false;
  return PLL_SUCCESS;
}

// the launches of resident schedule `dp` on e's stream (wgs: workgroups per CU and row, 0: the launcher's choice)
static int launch_resident(Engine * e, const ChainFamily & f, const DevicePlan & dp, const PlanView & view, unsigned wgs,
                           bool wide, bool transient)
{
  // (a storing schedule that defers stores but has neither folds nor looked-up children -- a caterpillar, many partial
  // lists -- runs the instantiation of evaluate-only traversals: the plain one does not read PlanOp::flags bit 0)
  const bool unstored = transient || (dp.ndeferred && !dp.nfolds && !dp.nlookups);
  for (const DevicePlan::Launch & l : dp.launches)
    if (!counted_launch(e, l.bytes, l.flops, l.ops, l.min_bytes, [&]()
        { return f.traverse(e, view, dp.lds_doubles, dp.max_extent, l.begin, l.end, l.rows, wgs, wide, unstored, dp.nfolds != 0, dp.nlookups != 0); }))
      return PLL_FAILURE;
  return PLL_SUCCESS;
}

// the list through the resident schedule prepare_schedule made for it: class operations and row tables, then the
// chains
static int run_resident(Engine * e, const ChainFamily & f, const pll_operation_t * ops, unsigned count, const RepeatPlan & rp,
                        bool transient)
{
  DevicePlan & dp = e->plan;
  PlanView view;
  if (!upload_plan(dp, e->stream, view)) return PLL_FAILURE;
  if (dp.ncherry_jobs || dp.npair_jobs)
  {
    if (!launch_class_levels(e, f, dp)) return PLL_FAILURE;
    // the scale buffers of the class operations hold their counts per class from now on (need_scaler)
    if (rp.active)
      for (unsigned k : rp.cherry_ops)
        if (ops[k].parent_scaler_index >= 0) e->scaler_lazy[ops[k].parent_scaler_index] = (int)ops[k].parent_clv_index;
    if (!dp.nlookups)                             // (the statistics of site repeats: not the tables of looked-up children)
    {
      e->repeat_stats.cherries += dp.ncherry_jobs;
      e->repeat_stats.classes += dp.repeat_classes;
      e->repeat_stats.sites += (unsigned long long)dp.ncherry_jobs * e->N;
    }
  }
  if (!launch_resident(e, f, dp, view, 0, !e->cherries.empty(), transient)) return PLL_FAILURE;
  // (a storing schedule marks only the stores it deferred: plan_defers)
  if (transient || dp.ndeferred) record_unstored(e, ops, count, dp, transient ? TRANSIENT_MODE : TRANSIENT_DEFERRED);
  // what became of the vectors that the deferring lists before this one left out: all given up unread -- the row of
  // such lists grows by this one --, or some stored for a reader -- a new row starts here (the family's default level
  // goes by its length: s20_defer; lists that leave nothing out -- the single operations of a smoothing pass -- say
  // nothing about it)
  if (dp.ndeferred) e->ledger.deferring_list_ran();
  count_list(e, count);
  return PLL_SUCCESS;
}

// the chains by value (ChainBatch, in the kernel arguments): one launch per round, longest chains first (their
// workgroups are dispatched first, which keeps the tail of the launch short)
static int run_chains_by_value(Engine * e, const ChainFamily & f, const pll_operation_t * ops, unsigned count,
                               unsigned lut_used, const ChainPlan & plan)
{
  for (int round = 0; round < plan.rounds; ++round)
  {
    ChainBatch cb;
    unsigned nops = 0, nchains = 0, longest = 0, lds = 0;
    double bytes = 0.0, flops = 0.0, minb = 0.0;
    auto flush = [&]() -> int
    {
      if (!nchains) return PLL_SUCCESS;
      if (!counted_launch(e, bytes, flops, nops, bytes - minb, [&]() -> int
          {
            if (longest > 1) return f.chains(e, cb, nchains, lds, lut_used);
            OpBatch ob;                       // nothing to hand over: the plain kernel
            for (unsigned i = 0; i < nops; ++i) ob.op[i] = cb.op[i];
            return launch_partials(e, ob, nops);
          }))
        return PLL_FAILURE;
      nops = nchains = longest = lds = 0;
      bytes = flops = minb = 0.0;
      return PLL_SUCCESS;
    };
    std::vector<size_t> order;
    for (size_t c = 0; c < plan.chains.size(); ++c)
      if (plan.launch[c] == round) order.push_back(c);
    std::stable_sort(order.begin(), order.end(),
                     [&](size_t a, size_t b) { return plan.chains[a].size() > plan.chains[b].size(); });
    for (size_t c : order)
    {
      const std::vector<unsigned> & ch = plan.chains[c];
      if (nops + ch.size() > MAX_OPS_PER_LAUNCH && !flush()) return PLL_FAILURE;
      cb.first[nchains] = (unsigned char)nops;
      cb.len[nchains] = (unsigned char)ch.size();
      unsigned off = 0;
      for (size_t i = 0; i < ch.size(); ++i)
      {
        const pll_operation_t & o = ops[ch[i]];
        if (!need_clv(e, o.child1_clv_index) || !need_clv(e, o.child2_clv_index)) return PLL_FAILURE;
        fill_desc(e, o, cb.op[nops], bytes, flops);
        cb.carried[nops] = i ? plan.carried[ch[i]] : 0;
        if (cb.carried[nops])       // handed over in registers: not read
          minb += (double)e->N * e->R * 8.0 * e->S +
                  ((cb.carried[nops] == 1 ? cb.op[nops].scaler1 : cb.op[nops].scaler2) ? 4.0 * (double)e->N * (e->rate_scalers ? e->R : 1) : 0.0);
        cb.slot1[nops] = (unsigned short)off;
        off += child_table_lds(e, f, o.child1_clv_index, lut_used, false);
        cb.slot2[nops] = (unsigned short)off;
        off += child_table_lds(e, f, o.child2_clv_index, lut_used, false);
        ++nops;
      }
      lds = std::max(lds, f.lds_is_length ? (unsigned)ch.size() : off);
      ++nchains;
      longest = std::max<unsigned>(longest, (unsigned)ch.size());
    }
    if (!flush()) return PLL_FAILURE;
  }
  count_list(e, count);
  return PLL_SUCCESS;
}

struct LevelPlan
{
  std::vector<int> level;                        // per op (-1: folded into its consumer)
  int max_level = 0;
  std::vector<char> light;                       // per op: runs behind the matrix-bound operations of its launch
  std::vector<int> cherry_of;                    // consumer -> the cherry folded into it
  std::vector<const uint8_t *> cherry_table;     // per folded cherry with a scale buffer: its scaling per pair of tip codes
  bool folding = false;
};

// 61 states.  (1) Cherries -- tip x tip operations, bound by HBM writes while the matrix cores
// idle -- are folded into the operation that consumes them (kernels_s61.hpp, k_partials_s61v4).
// (2) Those that stay (their consumer already folds its other child) run as LATE as the consumer
// allows, so that they share a launch with matrix-bound operations.  Both only for lists with the
// shape of a tree traversal (analyse_list); PLLHIP_S61_CHERRIES=0 / PLLHIP_S61_ALAP=0 switch
// them off.
static int fold_s61_cherries(Engine * e, const pll_operation_t * ops, unsigned count, LevelPlan & lp)
{
  static const int use_alap = getenv("PLLHIP_S61_ALAP") ? atoi(getenv("PLLHIP_S61_ALAP")) : 1;
  const PlannedList shape(e, nullptr, ops, count, 1u);
  if (!shape.accepted) return PLL_SUCCESS;
  const std::vector<int> & producer = shape.facts.producer, & consumer = shape.facts.consumer;
  auto is_cherry = [&](unsigned k) { return tip_coded(e, ops[k].child1_clv_index) && tip_coded(e, ops[k].child2_clv_index); };
  std::vector<char> folded(count, 0);
  if (s61_cherries_supported(e))
  {
    for (unsigned k = 0; k < count; ++k)
      if (is_cherry(k) && consumer[k] >= 0 && lp.cherry_of[consumer[k]] < 0)
      {
        lp.cherry_of[consumer[k]] = (int)k;
        folded[k] = 1;
        lp.folding = true;
      }
  }
  if (lp.folding)
  {
    // levels from the remaining dependencies alone (the list is a tree traversal: every vector
    // is written once and read by one later operation)
    lp.max_level = 0;
    for (unsigned k = 0; k < count; ++k)
    {
      if (folded[k]) { lp.level[k] = -1; continue; }
      int l = 0;
      for (int p : {producer[2 * k], producer[2 * k + 1]})
        if (p >= 0 && !folded[p]) l = std::max(l, lp.level[p] + 1);
      lp.level[k] = l;
      lp.max_level = std::max(lp.max_level, l);
    }
    // scaling decision of every folded cherry per pair of tip codes
    std::vector<unsigned> need;
    for (unsigned k = 0; k < count; ++k)
      if (folded[k] && ops[k].parent_scaler_index != PLL_SCALE_BUFFER_NONE) need.push_back(k);
    const size_t tab = (size_t)e->lut_codes * e->lut_codes;
    const size_t lut_stride = (size_t)e->R * e->lut_codes * e->S;
    if (need.size() * tab > e->s61_ttscale_cap)
    {
      PLLHIP_TRY(hipStreamSynchronize(e->stream));
      (void)hipFree(e->d_s61_ttscale);
      e->d_s61_ttscale = nullptr;
      e->s61_ttscale_cap = 0;
      if (!dev_alloc(&e->d_s61_ttscale, 2 * need.size() * tab, "cherry scaling tables")) return PLL_FAILURE;
      e->s61_ttscale_cap = 2 * need.size() * tab;
    }
    for (size_t i0 = 0; i0 < need.size(); i0 += 32)
    {
      CherryScaleBatch cs;
      memset(&cs, 0, sizeof(cs));
      const unsigned nc = (unsigned)std::min<size_t>(32, need.size() - i0);
      for (unsigned i = 0; i < nc; ++i)
      {
        const pll_operation_t & o = ops[need[i0 + i]];
        cs.lut1[i] = e->d_lut + lut_stride * o.child1_matrix_index;
        cs.lut2[i] = e->d_lut + lut_stride * o.child2_matrix_index;
        cs.out[i] = e->d_s61_ttscale + (i0 + i) * tab;
        lp.cherry_table[need[i0 + i]] = cs.out[i];
      }
      if (!launch_cherry_scale_s61(e, cs, nc)) return PLL_FAILURE;
    }
  }
  if (use_alap)
    for (unsigned k = 0; k < count; ++k)
    {
      if (folded[k] || !is_cherry(k)) continue;
      if (consumer[k] >= 0 && lp.level[consumer[k]] - 1 > lp.level[k]) lp.level[k] = lp.level[consumer[k]] - 1;
      lp.light[k] = 1;
    }
  return PLL_SUCCESS;
}

// dependency levels: an op runs after the producers of its children and after every earlier op that touched its
// output buffers (61 states: then fold_s61_cherries)
static int plan_levels(Engine * e, const pll_operation_t * ops, unsigned count, LevelPlan & lp)
{
  std::vector<int> clv_level(e->nodes, -1), sc_level(e->nscalers, -1);
  lp.level.assign(count, 0);
  lp.light.assign(count, 0);
  lp.cherry_of.assign(count, -1);
  lp.cherry_table.assign(count, nullptr);
  for (unsigned k = 0; k < count; ++k)
  {
    const pll_operation_t & op = ops[k];
    int l = 0;
    l = std::max(l, clv_level[op.child1_clv_index] + 1);
    l = std::max(l, clv_level[op.child2_clv_index] + 1);
    l = std::max(l, clv_level[op.parent_clv_index] + 1);
    if (op.child1_scaler_index >= 0) l = std::max(l, sc_level[op.child1_scaler_index] + 1);
    if (op.child2_scaler_index >= 0) l = std::max(l, sc_level[op.child2_scaler_index] + 1);
    if (op.parent_scaler_index >= 0) l = std::max(l, sc_level[op.parent_scaler_index] + 1);
    // every buffer touched (read or written) is stamped with this level, so any
    // later op that touches it again runs in a later launch.  In a tree
    // traversal a CLV is touched by its producer and its single consumer only,
    // so this costs no parallelism and covers RAW, WAR and WAW alike.
    lp.level[k] = l;
    clv_level[op.parent_clv_index] = l;
    clv_level[op.child1_clv_index] = std::max(clv_level[op.child1_clv_index], l);
    clv_level[op.child2_clv_index] = std::max(clv_level[op.child2_clv_index], l);
    if (op.parent_scaler_index >= 0) sc_level[op.parent_scaler_index] = l;
    if (op.child1_scaler_index >= 0)
      sc_level[op.child1_scaler_index] = std::max(sc_level[op.child1_scaler_index], l);
    if (op.child2_scaler_index >= 0)
      sc_level[op.child2_scaler_index] = std::max(sc_level[op.child2_scaler_index], l);
    lp.max_level = std::max(lp.max_level, l);
  }
  if (e->family == KernelFamily::S61 && lut_active(e) && count >= 2) return fold_s61_cherries(e, ops, count, lp);
  return PLL_SUCCESS;
}

// one launch per level, at most MAX_OPS_PER_LAUNCH operations (S61_V4_OPS when cherries are folded) each
static int run_levels(Engine * e, const pll_operation_t * ops, unsigned count, const LevelPlan & lp)
{
  for (int l = 0; l <= lp.max_level; ++l)
  {
    OpBatch batch, cherries;
    const uint8_t * tables[MAX_OPS_PER_LAUNCH];
    unsigned nb = 0, nfolded = 0;
    bool any_cherry = false;
    double batch_bytes = 0.0, batch_flops = 0.0;
    const unsigned cap = lp.folding ? S61_V4_OPS : MAX_OPS_PER_LAUNCH;
    // matrix-bound operations first, the light ones behind them (their workgroups fill the tail)
    for (unsigned pass = 0; pass < 2; ++pass)
    for (unsigned k = 0; k <= count; ++k)
    {
      if (k < count && (lp.light[k] != (char)pass)) continue;
      if (k == count && pass == 0) continue;
      if (k < count && lp.level[k] == l)
      {
        pll_operation_t o = ops[k];
        if (!need_clv(e, o.child1_clv_index) || !need_clv(e, o.child2_clv_index)) return PLL_FAILURE;
        memset(&cherries.op[nb], 0, sizeof(OpDesc));
        tables[nb] = nullptr;
        if (lp.cherry_of[k] >= 0)
        {
          const pll_operation_t & c = ops[lp.cherry_of[k]];
          if (o.child2_clv_index == c.parent_clv_index)      // the folded cherry is child 1 (products commute)
          {
            std::swap(o.child1_clv_index, o.child2_clv_index);
            std::swap(o.child1_matrix_index, o.child2_matrix_index);
            std::swap(o.child1_scaler_index, o.child2_scaler_index);
          }
          fill_desc(e, c, cherries.op[nb], batch_bytes, batch_flops);
          tables[nb] = lp.cherry_table[lp.cherry_of[k]];
          any_cherry = true;
          ++nfolded;
        }
        fill_desc(e, o, batch.op[nb++], batch_bytes, batch_flops);
      }
      if (nb == cap || (k == count && nb))
      {
        // (with cherries folded somewhere in the traversal, every launch takes the 512-thread kernel: 0.5 - 3 % faster
        // than switching to the 256-thread one for launches without a cherry)
        static const int all_v4 = getenv("PLLHIP_S61_ALLV4") ? atoi(getenv("PLLHIP_S61_ALLV4")) : 1;
        if (!counted_launch(e, batch_bytes, batch_flops, nb + nfolded, batch_bytes, [&]()
            {
              return (any_cherry || (all_v4 && lp.folding)) ? launch_partials_s61_cherries(e, batch, cherries, tables, nb)
                                                            : launch_partials(e, batch, nb);
            }))
          return PLL_FAILURE;
        nb = nfolded = 0;
        any_cherry = false;
        batch_bytes = 0.0;
        batch_flops = 0.0;
      }
    }
  }
  count_list(e, count);
  return PLL_SUCCESS;
}

static int update_partials_impl(pll_partition_t * p, const pll_operation_t * ops, unsigned count)
{
  Engine * e = engine_of(p);
  if (!begin_list(e, p, ops, count)) return PLL_FAILURE;
  // chain schedules (ChainFamily): the vector of a link stays in registers
  const ChainFamily * f = count >= 2 ? chain_family(e) : nullptr;
  // (tip tables are staged with the codes in use: at least one, an untouched partition)
  const unsigned lut_used = f ? std::max(1u, std::min(codes_in_use(e, p), e->lut_codes)) : 0u;
  const int mode = f ? resident_mode(e, *f, count) : -1;
  if (mode >= 0)
  {
    RepeatPlan rp;
    if (!select_class_ops(e, ops, count, lut_used, rp)) return PLL_FAILURE;
    // (evaluate-only traversals: not together with site repeats, whose class operations leave the list)
    const bool transient = e->transient_mode && !e->site_repeats;
    if (prepare_schedule(e, p, *f, {ops, count, (unsigned)mode, transient, rp.active ? &rp : nullptr, true}))
      return run_resident(e, *f, ops, count, rp, transient);
    if (rp.active)
      for (unsigned k : rp.cherry_ops) e->cherries[ops[k].parent_clv_index].valid = false;     // the plain paths below compute them
  }
  if (!plain_scalers(e, ops, count)) return PLL_FAILURE;
  if (f && f->chains)
  {
    const PlannedList pl(e, f, ops, count, lut_used);
    if (pl.accepted)
    {
      ChainPlan plan;
      plan_chains(pl.list, pl.facts, f->chain_max, f->chain_lds, plan);
      return run_chains_by_value(e, *f, ops, count, lut_used, plan);
    }
  }
  LevelPlan lp;
  if (!plan_levels(e, ops, count, lp)) return PLL_FAILURE;
  return run_levels(e, ops, count, lp);
}
} // namespace pllhip


namespace pllhip {

// ---------------------------------------------------------------------------
// One operation list over several partitions (pllhip_update_partials_batch).
// pll-modules evaluates every partition of an analysis on the same tree, one after the other
// (src/tree/treeinfo.c:1020-1056); with one partition per gene a partition holds a few thousand sites
// and every launch of its own costs more than it computes.  Partitions of one kernel family on one
// device share their launches instead: the round schedules of the members (prepare_schedule) are laid
// side by side in ONE resident schedule -- the chains of a round of every member become grid rows of the
// same launch, a chain knows its partition's extent and tables (PlanChain) -- on the first member's stream,
// with one event per member on either side.  What is stored is what the per-partition calls store,
// bit for bit: the same kernels run the same chains.
// ---------------------------------------------------------------------------
static bool batch_family(const Engine * e)
{
  static const int use_batch = getenv("PLLHIP_BATCH") ? atoi(getenv("PLLHIP_BATCH")) : 1;
  if (!use_batch || !e->shards.empty() || e->site_repeats) return false;
  return chain_family(e) != nullptr;
}

static bool batch_compatible(const Engine * a, const Engine * b)
{
  return a->device == b->device && a->family == b->family && a->S == b->S && a->R == b->R &&
         a->rate_scalers == b->rate_scalers;
}

static void batch_free(BatchPlan * b)
{
  if (!b) return;
  (void)hipFree(b->plan.d_buf);
  if (b->plan.h_stage) (void)hipHostFree(b->plan.h_stage);
  if (b->plan.copied) (void)hipEventDestroy(b->plan.copied);
  for (hipEvent_t ev : b->ready) if (ev) (void)hipEventDestroy(ev);
  if (b->done) (void)hipEventDestroy(b->done);
  delete b;
}

// 1 = done as one batch, 0 = the members' schedules cannot share launches (the caller falls back to
// per-partition calls), -1 = error
static int update_partials_group(const std::vector<pll_partition_t *> & g, const pll_operation_t * ops, unsigned count)
{
  Engine * lead = engine_of(g[0]);
  const ChainFamily & f = *chain_family(lead);       // (the members': batch_family, batch_compatible)
  const size_t M = g.size();
  if (hipSetDevice(lead->device) != hipSuccess) { set_error(PLL_ERROR_HIP_RUNTIME, "hipSetDevice"); return -1; }
  // One launch for the whole list (every member gets grid rows of its own, whose workgroups walk ALL chains
  // of the member for their share of its site blocks: no launch boundary, no tail between rounds), or one
  // launch per round of chains (the chains of a round of every member side by side)?  The first needs enough
  // site blocks in the group to fill the chip without the parallelism of the chains.  PLLHIP_BATCH_MODE=1 / 0.
  static const int env_mode = getenv("PLLHIP_BATCH_MODE") ? atoi(getenv("PLLHIP_BATCH_MODE")) : -1;
  unsigned long long units = 0;       // workgroups the members could use side by side
  for (pll_partition_t * p : g) units += f.units(engine_of(p));
  const unsigned mode = env_mode >= 0 ? (env_mode ? 1u : 0u) : (units >= 2ull * lead->cu_count && count >= 2) ? 1u : 0u;
  for (pll_partition_t * p : g)
  {
    Engine * e = engine_of(p);
    // (a member never has site repeats -- batch_family --, so none of the vectors this list writes is a valid class node
    // and the prologue's loop over them only writes them off; where a later member makes this function return 0, the
    // per-partition calls run the prologue on the earlier members again, and find nothing left to do)
    if (!begin_list(e, p, ops, count)) return -1;
    if (!prepare_schedule(e, p, f, {ops, count, mode, e->transient_mode && !e->site_repeats, nullptr})) return 0;
  }
  // launches can be shared when every member's schedule has the same shape (same list, same family: always,
  // unless the tables of one member fill the LDS earlier and cut its chains elsewhere)
  const DevicePlan & first = lead->plan;
  for (size_t m = 1; m < M; ++m)
  {
    const DevicePlan & dp = engine_of(g[m])->plan;
    if (dp.launches.size() != first.launches.size() || dp.nchains != first.nchains) return 0;
    for (size_t j = 0; j < dp.launches.size(); ++j)
      if (dp.launches[j].rows != first.launches[j].rows ||
          dp.launches[j].end - dp.launches[j].begin != first.launches[j].end - first.launches[j].begin)
        return 0;
  }

  if (!lead->batch) lead->batch = new BatchPlan();
  BatchPlan & b = *lead->batch;
  bool same = b.members.size() == M;
  for (size_t m = 0; same && m < M; ++m)
    same = b.members[m] == (const void *)engine_of(g[m]) && b.generations[m] == engine_of(g[m])->plan.generation;
  if (!same)
  {
    b.members.resize(M);
    b.generations.resize(M);
    DevicePlan & mp = b.plan;
    std::vector<PlanOp> pops;
    std::vector<PlanChain> pchains;
    std::vector<unsigned> base(M);
    mp.lds_doubles = 0;
    mp.max_extent = 0;
    for (size_t m = 0; m < M; ++m)
    {
      const DevicePlan & dp = engine_of(g[m])->plan;
      b.members[m] = engine_of(g[m]);
      b.generations[m] = dp.generation;
      base[m] = (unsigned)pops.size();
      const PlanOp * src = reinterpret_cast<const PlanOp *>(dp.bytes.data());
      pops.insert(pops.end(), src, src + dp.nops);
      mp.lds_doubles = std::max(mp.lds_doubles, dp.lds_doubles);
      mp.max_extent = std::max(mp.max_extent, dp.max_extent);
    }
    mp.launches.clear();
    for (size_t j = 0; j < first.launches.size(); ++j)
    {
      DevicePlan::Launch l = first.launches[j];
      const unsigned nch = l.end - l.begin;
      l.begin = (unsigned)pchains.size();
      l.ops = 0;
      l.bytes = l.flops = l.min_bytes = 0.0;
      // a round: the chains of every member side by side (a row each).  A run of single chains (rows == 1:
      // one row walks them in turn): step-major, so that with one row per member row m walks member m's chains
      const bool run = first.launches[j].rows == 1;
      const size_t row0 = pchains.size();
      for (unsigned x = 0; x < (run ? nch : (unsigned)M); ++x)
        for (unsigned y = 0; y < (run ? (unsigned)M : nch); ++y)
        {
          const size_t m = run ? y : x;
          const unsigned c = run ? x : y;
          const DevicePlan & dp = engine_of(g[m])->plan;
          const PlanChain * chains = reinterpret_cast<const PlanChain *>(dp.bytes.data() + (size_t)dp.nops * sizeof(PlanOp));
          PlanChain pc = chains[dp.launches[j].begin + c];
          pc.first += base[m];
          pchains.push_back(pc);
        }
      // the rows of a round are independent: the most expensive ones (operations x site blocks) are dispatched first,
      // whatever partition they belong to, which keeps the tail of the launch short
      if (!run)
        std::stable_sort(pchains.begin() + row0, pchains.end(), [](const PlanChain & a, const PlanChain & b)
        { return (unsigned long long)a.len * a.extent > (unsigned long long)b.len * b.extent; });
      for (size_t m = 0; m < M; ++m)
      {
        const DevicePlan::Launch & lm = engine_of(g[m])->plan.launches[j];
        l.ops += lm.ops; l.bytes += lm.bytes; l.flops += lm.flops; l.min_bytes += lm.min_bytes;
      }
      l.end = (unsigned)pchains.size();
      l.rows = first.launches[j].rows * (unsigned)M;
      mp.launches.push_back(l);
    }
    mp.nops = (unsigned)pops.size();
    mp.nchains = (unsigned)pchains.size();
    mp.bytes.resize(pops.size() * sizeof(PlanOp) + pchains.size() * sizeof(PlanChain));
    memcpy(mp.bytes.data(), pops.data(), pops.size() * sizeof(PlanOp));
    memcpy(mp.bytes.data() + pops.size() * sizeof(PlanOp), pchains.data(), pchains.size() * sizeof(PlanChain));
  }
  while (b.ready.size() < M)
  {
    hipEvent_t ev;
    if (!hip_ok(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate")) return -1;
    b.ready.push_back(ev);
  }
  if (!b.done && !hip_ok(hipEventCreateWithFlags(&b.done, hipEventDisableTiming), "hipEventCreate")) return -1;

  // the row tables of the members' wide tips (tips kept per class of sites), each on its member's stream
  bool any_wide = false;
  for (pll_partition_t * p : g)
  {
    Engine * e = engine_of(p);
    any_wide = any_wide || !e->cherries.empty();
    if (!e->plan.npair_jobs) continue;
    PlanView own;
    if (hipSetDevice(e->device) != hipSuccess || !upload_plan(e->plan, e->stream, own) || !launch_class_levels(e, f, e->plan)) return -1;
  }
  // the members' streams have issued what the traversal reads (P-matrices, tables, tip data)
  for (size_t m = 1; m < M; ++m)
    if (!hip_ok(hipEventRecord(b.ready[m], engine_of(g[m])->stream), "hipEventRecord") ||
        !hip_ok(hipStreamWaitEvent(lead->stream, b.ready[m], 0), "hipStreamWaitEvent"))
      return -1;
  PlanView view;
  if (!upload_plan(b.plan, lead->stream, view)) return -1;
  // one launch for the whole list: the rows are the members, every workgroup has the same long walk in front
  // of it, so exactly the workgroups that are resident at once (ChainFamily::batch_wgs per CU)
  static const int env_walk = getenv("PLLHIP_BATCH_WGS") ? atoi(getenv("PLLHIP_BATCH_WGS")) : 0;
  const unsigned wgs = mode ? (env_walk > 0 ? (unsigned)env_walk : f.batch_wgs) : 0u;
  bool any_transient = false;
  for (pll_partition_t * p : g) any_transient = any_transient || (engine_of(p)->transient_mode && !engine_of(p)->site_repeats);
  if (!launch_resident(lead, f, b.plan, view, wgs, any_wide, any_transient)) return -1;
  // whatever a member's stream does next comes after the traversal
  if (!hip_ok(hipEventRecord(b.done, lead->stream), "hipEventRecord")) return -1;
  for (size_t m = 1; m < M; ++m)
    if (!hip_ok(hipStreamWaitEvent(engine_of(g[m])->stream, b.done, 0), "hipStreamWaitEvent")) return -1;
  for (pll_partition_t * p : g)
  {
    Engine * e = engine_of(p);
    if (e->transient_mode && !e->site_repeats) record_unstored(e, ops, count, e->plan, TRANSIENT_MODE);
    count_list(e, count);
  }
  return 1;
}

} // namespace pllhip

extern "C" int pllhip_update_partials_batch(pll_partition_t * const * partitions, unsigned int partition_count,
                                            const pll_operation_t * ops, unsigned int count)
{
  using namespace pllhip;
  if (!count) return PLL_SUCCESS;
  int rc = PLL_SUCCESS;
  std::vector<char> taken(partition_count, 0);
  // the tip tables first: whether a partition's traversals can run from a shared schedule depends on their size
  // (chain_family reads lut_codes, the row count and not the contents: the 4-state chains want 16 rows).  Coming before
  // the queued P-matrices is no change of order: flush_pmatrices itself calls ensure_luts first where the tables are
  // stale, and the matrix kernel then fills the rows of what was queued.  Everything else -- unstored vectors, pending
  // P-matrices, class nodes -- is begin_list's, per member or per partition
  for (unsigned i = 0; i < partition_count; ++i)
    if (partitions[i] && !is_router(partitions[i]))
    {
      PLLHIP_TRY(hipSetDevice(engine_of(partitions[i])->device));
      if (!ensure_luts(partitions[i])) return PLL_FAILURE;
    }
  for (unsigned i = 0; i < partition_count; ++i)
  {
    if (!partitions[i] || taken[i]) continue;
    taken[i] = 1;
    std::vector<pll_partition_t *> group(1, partitions[i]);
    const Engine * e = engine_of(partitions[i]);
    if (batch_family(e))
      for (unsigned j = i + 1; j < partition_count; ++j)
        if (partitions[j] && !taken[j] && partitions[j] != partitions[i] && batch_family(engine_of(partitions[j])) &&
            batch_compatible(e, engine_of(partitions[j])))
        {
          taken[j] = 1;
          group.push_back(partitions[j]);
        }
    int done = 0;
    if (group.size() > 1)
    {
      done = update_partials_group(group, ops, count);
      if (done < 0) { rc = PLL_FAILURE; continue; }
    }
    if (!done)
      for (pll_partition_t * p : group)
      {
        pll_errno = 0;
        pll_update_partials(p, ops, count);
        if (pll_errno) rc = PLL_FAILURE;
      }
  }
  return rc;
}

namespace pllhip {

// ---------------------------------------------------------------------------
// router: a partition spread over several devices (Engine::shards)
// ---------------------------------------------------------------------------
// where a shard's next reduction leaves its totals: its own mapped result buffer
static Engine::Sink shard_sink(Engine * c)
{
  Engine::Sink sk;
  sk.dst = c->d_result;
  sk.flag = reinterpret_cast<unsigned long long *>(c->d_result) + RESULT_SEQ_SLOT;
  sk.seq = ++c->result_seq;
  sk.nq = 0;
  return sk;
}

static int shard_wait(Engine * c, unsigned long long seq)
{
  const volatile unsigned long long * flag =
      reinterpret_cast<const volatile unsigned long long *>(c->h_result) + RESULT_SEQ_SLOT;
  return wait_sequence(c->stream, flag, seq);
}

// every shard's kernel is enqueued (all devices run at once), then the totals are collected and
// added in shard order: bit-reproducible, whatever the devices' finishing order
static double router_loglikelihood(pll_partition_t * p, unsigned pc, int psc, unsigned cc, int csc,
                                   int matrix_index, const unsigned * freqs_indices, double * persite_lnl)
{
  Engine * r = engine_of(p);
  const double fail = -std::numeric_limits<double>::infinity();
  std::vector<unsigned long long> seq(r->shards.size());
  for (size_t k = 0; k < r->shards.size(); ++k)
  {
    pll_partition_t * c = r->shards[k];
    push_model(p, c);
    Engine::Sink sk = shard_sink(engine_of(c));
    seq[k] = sk.seq;
    const double v = loglikelihood_impl(c, pc, psc, cc, csc, matrix_index, freqs_indices,
                                        persite_lnl ? persite_lnl + r->shard_first[k] : nullptr, &sk);
    if (v != 0.0) return fail;
  }
  double total = 0.0;
  for (size_t k = 0; k < r->shards.size(); ++k)
  {
    Engine * c = engine_of(r->shards[k]);
    if (hipSetDevice(c->device) != hipSuccess || !shard_wait(c, seq[k])) return fail;
    if (persite_lnl && !hip_ok(hipStreamSynchronize(c->stream), "persite sync")) return fail;
    total += c->h_result[0];
  }
  return total;
}

static int router_derivatives(pll_partition_t * p, int psc, int csc, const double * brlens, unsigned count,
                              const unsigned * params_indices, const double * sumtable,
                              double * out_df, double * out_ddf)
{
  Engine * r = engine_of(p);
  std::vector<unsigned long long> seq(r->shards.size());
  for (size_t k = 0; k < r->shards.size(); ++k)
  {
    pll_partition_t * c = r->shards[k];
    push_model(p, c);
    Engine::Sink sk = shard_sink(engine_of(c));
    seq[k] = sk.seq;
    if (!derivatives_impl(c, psc, csc, brlens, count, params_indices, sumtable, &sk, nullptr, nullptr))
      return PLL_FAILURE;
  }
  for (unsigned i = 0; i < count; ++i) out_df[i] = out_ddf[i] = 0.0;
  for (size_t k = 0; k < r->shards.size(); ++k)
  {
    Engine * c = engine_of(r->shards[k]);
    PLLHIP_TRY(hipSetDevice(c->device));
    if (!shard_wait(c, seq[k])) return PLL_FAILURE;
    for (unsigned i = 0; i < count; ++i) { out_df[i] += c->h_result[2 * i]; out_ddf[i] += c->h_result[2 * i + 1]; }
  }
  return PLL_SUCCESS;
}

} // namespace pllhip

using namespace pllhip;

// ===========================================================================
// B0 entry points
// ===========================================================================
extern "C" {

int pll_update_prob_matrices(pll_partition_t * p,
                             const unsigned int * params_indices,
                             const unsigned int * matrix_indices,
                             const double * branch_lengths,
                             unsigned int count)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    // the decomposition runs once, on the parent's arrays; every shard builds the (tiny) matrices itself
    if (!ensure_eigen(p, params_indices)) return PLL_FAILURE;
    for (pll_partition_t * c : e->shards)
    {
      push_model(p, c);
      if (!pll_update_prob_matrices(c, params_indices, matrix_indices, branch_lengths, count)) return PLL_FAILURE;
    }
    return PLL_SUCCESS;
  }
  // (no HIP call on the queueing path: the reference issues one call per branch and partition -- 6 304 per
  // evaluation of 32 partitions on 100 taxa --; the device is selected where something is launched or copied)
  if (!ensure_eigen(p, params_indices)) return PLL_FAILURE;
  if (!sync_model(p, e->pmatrix_burst)) return PLL_FAILURE;
  e->pmatrix_burst = true;                    // until another entry point looks at the model
  for (unsigned m = 0; m < count; ++m)
    if (matrix_indices[m] >= e->nmat || !(branch_lengths[m] >= 0.0))
    {
      set_error(PLL_ERROR_PARAM_INVALID, "Invalid matrix index %u or branch length %g",
                matrix_indices[m], branch_lengths[m]);
      return PLL_FAILURE;
    }
  // queue; a request for a matrix that is already queued replaces it
  const ParamIdx params = make_params(p, params_indices);
  if (!e->pend_midx.empty() && memcmp(&params, &e->pend_params, sizeof(params)) != 0)
    if (!flush_pmatrices(p)) return PLL_FAILURE;
  e->pend_params = params;
  if (e->pend_pos.size() != e->nmat) e->pend_pos.assign(e->nmat, -1);
  for (unsigned m = 0; m < count; ++m)
  {
    const unsigned idx = matrix_indices[m];
    if (e->pend_pos[idx] >= 0)
      e->pend_t[e->pend_pos[idx]] = branch_lengths[m];
    else
    {
      e->pend_pos[idx] = (int)e->pend_midx.size();
      e->pend_midx.push_back(idx);
      e->pend_t.push_back(branch_lengths[m]);
    }
  }
  e->pmat_host_dirty = true;
  e->counters.pmatrix_updates += count;
  // every matrix of the partition is queued: no later request can join this launch (a repeated one replaces its
  // entry), so it goes now -- with several partitions the kernel of this one runs while the host issues the
  // per-branch calls of the next (src/tree/treeinfo.c:845-865 loops the partitions inside every branch)
  // (not while vectors exist as their operation only: the launch waits for the consumer -- if that is the next
  // traversal, it gives those vectors up before the matrices they were made with change; flush_pmatrices)
  if (e->ledger.empty() && (e->pend_midx.size() >= 4 * MAX_PMAT_PER_LAUNCH || e->pend_midx.size() == e->nmat)) return flush_pmatrices(p);
  return PLL_SUCCESS;
}

void pll_update_partials(pll_partition_t * p, const pll_operation_t * ops, unsigned int count)
{
  if (!count) return;
  // void in the reference interface: errors are reported through pll_errno
  if (is_router(p))
  {
    for (pll_partition_t * c : engine_of(p)->shards) (void)update_partials_impl(c, ops, count);
    return;
  }
  (void)update_partials_impl(p, ops, count);
}

} // extern "C"

namespace pllhip {

// lnL at an edge (matrix_index >= 0) or at a root vector.  `deferred` == nullptr: the
// value comes back (one wait); otherwise the total is left at deferred->dst (a device
// slot or mapped memory, with deferred->flag / seq if the host is to be told), nothing
// is waited for and the return value is 0.  `persite_dev` (blocking form only): device memory
// on this engine's device that receives the per-site values of the alignment patterns, copied
// on the engine's stream and not waited for.
double loglikelihood_impl(pll_partition_t * p, unsigned pc, int psc, unsigned cc, int csc,
                          int matrix_index, const unsigned * freqs_indices,
                          double * persite_lnl, const Engine::Sink * deferred, double * persite_dev)
{
  Engine * e = engine_of(p);
  const double fail = -std::numeric_limits<double>::infinity();
  if (hipSetDevice(e->device) != hipSuccess) { set_error(PLL_ERROR_HIP_RUNTIME, "hipSetDevice"); return fail; }
  if (!check_clv_index(e, pc, "parent") || !check_scaler_index(e, psc)) return fail;
  if (matrix_index >= 0)
  {
    if (!check_clv_index(e, cc, "child") || !check_scaler_index(e, csc)) return fail;
    if ((unsigned)matrix_index >= e->nmat) { set_error(PLL_ERROR_PARAM_INVALID, "matrix index out of range"); return fail; }
  }
  if (!sync_model(p) || !flush_pmatrices(p) || !ensure_luts(p) || !ensure_invariant(p)) return fail;
  if (!need_clv(e, pc) || (matrix_index >= 0 && !need_clv(e, cc))) return fail;
  if (!need_scaler(e, psc) || (matrix_index >= 0 && !need_scaler(e, csc))) return fail;
  // ascertainment-bias correction: the kernel runs over alignment + constant patterns (the
  // latter weigh 0 on the device), the per-site values of the constant patterns come back
  // through the mapped result buffer and the host adds the closed-form correction
  const bool asc = e->N > e->Nreal;
  if (asc && deferred)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "internal: deferred lnL of an AB partition goes through the blocking form");
    return fail;
  }
  double * const ps_out_req = persite_lnl;
  if ((persite_lnl || persite_dev || asc) && !e->d_persite)
    if (!dev_alloc(&e->d_persite, (size_t)e->N, "per-site lnL")) return fail;
  if (asc && !persite_lnl) persite_lnl = e->h_asc;      // any non-null value: "per-site output on"

  const unsigned nblocks = reduce_grid(e);
  const ModelView mv = model_view(e);
  const ParamIdx fidx = make_params(p, freqs_indices);
  const NodeRef parent = node_ref(e, pc);
  if (deferred) e->sink = *deferred; else sink_to_host(e);
  e->sink.nq = 1;
  unsigned long long * const host_flag = e->sink.flag;
  if (asc) e->sink.flag = nullptr;                      // k_publish_tail tells the host, after the tail
  NodeRef child = {nullptr, nullptr};
  const double * pm = nullptr, * lut = nullptr;
  if (matrix_index >= 0)
  {
    child = node_ref(e, cc);
    pm = e->d_pmat + (size_t)matrix_index * e->R * e->S * e->Sp;
    if (child.codes) lut = e->d_lut + (size_t)matrix_index * e->R * e->lut_codes * e->S;
  }
  const EdgeFamily * f = edge_family(e);
  const bool edge = matrix_index >= 0;
  if (!(edge ? f->lnl : f->root_lnl)(e, mv, fidx, parent, child, pm, lut, scaler_ptr(e, psc),
                                      (edge || f->root_child_scaler) ? scaler_ptr(e, csc) : nullptr,
                                      (persite_lnl || persite_dev) ? e->d_persite : nullptr, nblocks)) return fail;
  double total = 0.0;
  e->counters.lnl_calls++;
  if (deferred)
  {
    if (!finish_launch(e, nblocks, 1)) return fail;
    // (the caller waits for the stream before it reads a per-site buffer)
    if (ps_out_req && e->Nreal &&
        !hip_ok(hipMemcpyAsync(ps_out_req, e->d_persite, sizeof(double) * e->Nreal, hipMemcpyDeviceToHost, e->stream),
                "persite copy")) return fail;
    return 0.0;
  }
  if (asc)
  {
    if (!finish_launch(e, nblocks, 1)) return fail;
    hipLaunchKernelGGL(k_publish_tail, dim3(1), dim3(64), 0, e->stream, e->d_persite + e->Nreal,
                       e->d_result + RESULT_ASC_SLOT, e->S, host_flag, e->sink.seq);
    if (!hip_ok(hipGetLastError(), "publish tail")) return fail;
    const volatile unsigned long long * flag =
        reinterpret_cast<const volatile unsigned long long *>(e->h_result) + RESULT_SEQ_SLOT;
    if (!wait_sequence(e->stream, flag, e->sink.seq)) return fail;
    total = e->h_result[0] + asc_correction(p, e->h_result + RESULT_ASC_SLOT);
  }
  else if (!finish_reduction(e, nblocks, 1, &total)) return fail;
  if (ps_out_req && e->Nreal)
  {
    // only the alignment patterns go to the caller; wait for the copy (the result flag came first)
    if (!hip_ok(hipMemcpyAsync(ps_out_req, e->d_persite, sizeof(double) * e->Nreal,
                               hipMemcpyDeviceToHost, e->stream), "persite copy") ||
        !hip_ok(hipStreamSynchronize(e->stream), "persite sync")) return fail;
  }
  // a site-likelihood set (pll_rell_dev.hip) takes the alignment patterns on the device, in stream order
  if (persite_dev && e->Nreal &&
      !hip_ok(hipMemcpyAsync(persite_dev, e->d_persite, sizeof(double) * e->Nreal, hipMemcpyDeviceToDevice, e->stream),
              "persite device copy")) return fail;
  return total;
}

// PLLHIP_NEWTON_RESIDENT=0: no loop keeps the sumtable in registers
static bool newton_resident_enabled()
{
  static const int env_res = getenv("PLLHIP_NEWTON_RESIDENT") ? atoi(getenv("PLLHIP_NEWTON_RESIDENT")) : 1;
  return env_res != 0;
}

// 4 states (kernels_newton_s4.hpp): the loop with the table in registers when a thread has at most two trips on the grid
// that variant can hold at once; otherwise the host loop (capacity 0: a streaming loop in one launch measured no faster
// than one blocking call per iterate -- 59.3 against 57.7 us all-in at 1 M sites)
static bool newton_probe_s4(Engine * e)
{
  const void * fn2 = reinterpret_cast<const void *>(k_newton_s4<2>);
  int cu2 = 0;
  if (!hip_ok(hipOccupancyMaxActiveBlocksPerMultiprocessor(&cu2, fn2, 256, 0), "hipOccupancyMaxActiveBlocksPerMultiprocessor"))
    return false;
  const unsigned cap2 = (unsigned)std::max(0, cu2) * e->cu_count;
  const unsigned long long limit = ((unsigned long long)e->N * e->R + 63ULL) & ~63ULL;
  // (the grid the loop is launched on: scan_grid() = the reduction grid, at most four workgroups per CU and at
  // most what the chip holds at once)
  const unsigned g2 = std::min({reduce_grid(e), 4u * e->cu_count, cap2});
  const bool resident = newton_resident_enabled() && g2 && (limit + 1024ULL * g2 - 1) / (1024ULL * g2) <= 2;
  e->newton_resident = resident ? 2 : 0;
  // (newton_prepare takes the stream fields for a loop over several partitions: at 4 states that form is this one)
  e->newton_fn = e->newton_stream_fn = fn2;
  e->newton_lds = e->newton_stream_lds = 0;
  e->newton_capacity = e->newton_stream_capacity = resident ? (int)cap2 : 0;
  return true;
}

// the register-resident form of a matrix-core loop: `nb` site blocks per wave, its LDS beyond the streaming loop's
struct NewtonResident { const void * fn; unsigned nb; size_t extra_lds; };

// the matrix cores: the streaming loop `fn` at `ks` k-steps, and the family's register-resident candidate
static bool newton_probe_mfma(Engine * e, unsigned ks, const void * fn, const NewtonResident & res)
{
  const size_t lds = newton_table_lds(e, ks);
  e->newton_resident = 0;
  e->newton_fn = fn;
  e->newton_lds = lds;
  if (lds > 160 * 1024 - 512) { e->newton_capacity = 0; return true; }
  if (lds > 64 * 1024 && !hip_ok(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512), "hipFuncSetAttribute"))
    return false;
  int per_cu = 0;
  if (!hip_ok(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds), "hipOccupancyMaxActiveBlocksPerMultiprocessor"))
    return false;
  e->newton_capacity = std::max(0, per_cu) * (int)e->cu_count;
  e->newton_stream_fn = fn;
  e->newton_stream_lds = lds;
  e->newton_stream_capacity = e->newton_capacity;
  // Does the sumtable fit the registers of the waves of ONE co-resident grid (k_newton_mfma_resident)?  Then that
  // grid is the scan grid of this partition -- for the single scans of derivatives_impl as well, so that both
  // add the same block totals in the same order.
  if (!newton_resident_enabled() || !res.fn || e->R != 4 || e->rate_scalers || lds > 64 * 1024) return true;
  const size_t res_lds = lds + res.extra_lds;
  int res_cu = 0;
  if (res_lds > 64 * 1024 && !hip_ok(hipFuncSetAttribute(res.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)res_lds), "hipFuncSetAttribute"))
    return false;
  if (!hip_ok(hipOccupancyMaxActiveBlocksPerMultiprocessor(&res_cu, res.fn, 256, res_lds), "hipOccupancyMaxActiveBlocksPerMultiprocessor"))
    return false;
  const unsigned cap_res = (unsigned)std::max(0, res_cu) * e->cu_count;
  const unsigned g = std::min({reduce_grid(e), 4u * e->cu_count, cap_res});
  if (g && (unsigned long long)e->nblk <= (unsigned long long)res.nb * 4u * g)
  {
    e->newton_resident = (int)res.nb;
    e->newton_fn = res.fn;
    e->newton_lds = res_lds;
    e->newton_capacity = (int)cap_res;
  }
  return true;
}

static bool newton_probe_s20(Engine * e)
{
  return newton_probe_mfma(e, 5, reinterpret_cast<const void *>(k_newton_mfma<5, 20>),
                           {reinterpret_cast<const void *>(k_newton_mfma_resident<5, 20, 4, 3>), 4, sizeof(double2) * 4 * 4 * 5 * 64});
}

static bool newton_probe_s61(Engine * e)
{
  if (e->S == S61_S)
    return newton_probe_mfma(e, S61_KS, reinterpret_cast<const void *>(k_newton_mfma<S61_KS, S61_S>),
                             {reinterpret_cast<const void *>(k_newton_mfma_resident<S61_KS, S61_S, 1, 1>), 1, 0});
  return newton_probe_mfma(e, S61_KS, reinterpret_cast<const void *>(k_newton_mfma<S61_KS, 0>),
                           {reinterpret_cast<const void *>(k_newton_mfma_resident<S61_KS, 0, 1, 1>), 1, 0});
}

// 2 .. 32 states: site blocks that k_newton_mfma_resident keeps in registers at KS k-steps -- as many as ~240 registers
// hold (16 KS per block) --, one more in LDS
constexpr unsigned S16_RESIDENT_BLOCKS[9] = {0, 7, 7, 5, 3, 3, 2, 2, 1};

static bool newton_probe_s16(Engine * e)
{
  const void * fn = nullptr;
  NewtonResident res = {nullptr, 0, 0};
#define PLLHIP_STREAMING(KK) fn = reinterpret_cast<const void *>(k_newton_mfma<KK, 0>)
#define PLLHIP_RESIDENT(KK) \
  res = {reinterpret_cast<const void *>(k_newton_mfma_resident<KK, 0, S16_RESIDENT_BLOCKS[KK] + 1, S16_RESIDENT_BLOCKS[KK]>), \
         S16_RESIDENT_BLOCKS[KK] + 1, sizeof(double2) * 4 * 4 * KK * 64}
  PLLHIP_DISPATCH_KS(s16_ks(e), PLLHIP_STREAMING);
  PLLHIP_DISPATCH_KS(s16_ks(e), PLLHIP_RESIDENT);
#undef PLLHIP_STREAMING
#undef PLLHIP_RESIDENT
  return newton_probe_mfma(e, s16_ks(e), fn, res);
}

// how many workgroups of the family's loop kernel (Engine::newton_fn, newton_lds) the chip holds at once (-1: HIP error).
// derivatives_impl sizes its scan grid with the same number, so that the device loop and the host loop add the same
// block totals in the same order.
static int newton_capacity(Engine * e)
{
  if (e->newton_capacity < 0 && !edge_family(e)->newton_probe(e)) return -1;
  return e->newton_capacity;
}

// workgroups of a derivative scan on the matrix cores: long-lived ones (the scan pipelines its loads across the
// units a wave walks; tables built, totals reduced and published less often), and no more than the chip holds at
// once, so that pllhip_newton_branch can run the very same grid as a loop
static unsigned scan_grid(Engine * e)
{
  unsigned nblocks = std::min(reduce_grid(e), 4u * e->cu_count);
  const int cap = newton_capacity(e);
  if (cap > 0) nblocks = std::min(nblocks, (unsigned)cap);
  return nblocks;
}

// K = up to MAX_TRIAL_LENGTHS trial branch lengths per sumtable scan; totals in the order
// df[0], ddf[0], df[1], ddf[1], ...  (to out_df / out_ddf, or left at deferred->dst)
int derivatives_impl(pll_partition_t * p, int parent_scaler_index, int child_scaler_index,
                     const double * brlens, unsigned count, const unsigned * params_indices,
                     const double * sumtable, const Engine::Sink * deferred,
                     double * out_df, double * out_ddf)
{
  Engine * e = engine_of(p);
  PLLHIP_TRY(hipSetDevice(e->device));
  if (!check_scaler_index(e, parent_scaler_index) || !check_scaler_index(e, child_scaler_index))
    return PLL_FAILURE;
  if (!count || count > MAX_TRIAL_LENGTHS)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "1 to %u trial branch lengths per call", MAX_TRIAL_LENGTHS);
    return PLL_FAILURE;
  }
  double * d_sum = sumtable_device(e, sumtable, false);
  if (!d_sum)
  {
    set_error(PLL_ERROR_PARAM_INVALID,
              "pll_compute_likelihood_derivatives: no sumtable was computed for this buffer");
    return PLL_FAILURE;
  }
  if (!sync_model(p) || !ensure_invariant(p)) return PLL_FAILURE;
  if (!need_scaler(e, parent_scaler_index) || !need_scaler(e, child_scaler_index)) return PLL_FAILURE;
  const EdgeFamily * f = edge_family(e);
  const unsigned nblocks = f->scan_on_newton_grid ? scan_grid(e) : reduce_grid(e);
  const ModelView mv = model_view(e);
  const ParamIdx params = make_params(p, params_indices);
  const unsigned kmax = f->trial_lengths(e);
  if (!kmax) return PLL_FAILURE;
  const bool asc = e->N > e->Nreal;
  if (asc && deferred)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "internal: deferred derivatives of an AB partition go through the blocking form");
    return PLL_FAILURE;
  }
  if (asc)
  {
    // {A, B, C, count} of the constant patterns at every trial length, ahead of the scan on the
    // same stream: when the scan's result flag arrives these are in host memory too
    TrialLengths all;
    for (unsigned i = 0; i < MAX_TRIAL_LENGTHS; ++i) all.t[i] = brlens[std::min(i, count - 1)];
    hipLaunchKernelGGL(k_asc_abc, dim3(1), dim3(256), 0, e->stream, mv, params, all, count, d_sum,
                       scaler_ptr(e, parent_scaler_index), scaler_ptr(e, child_scaler_index),
                       e->Nreal, e->R, e->rows, e->rate_scalers ? 1u : 0u, e->d_asc);
    PLLHIP_TRY(hipGetLastError());
  }
  Engine::Sink base;
  if (deferred) base = *deferred; else { sink_to_host(e); base = e->sink; }
  for (unsigned first = 0; first < count; first += kmax)
  {
    const unsigned nb = std::min(kmax, count - first);
    TrialLengths tl;
    for (unsigned i = 0; i < MAX_TRIAL_LENGTHS; ++i) tl.t[i] = brlens[first + std::min(i, nb - 1)];
    e->sink = base;
    e->sink.dst = base.dst + 2 * first;
    e->sink.nq = 2 * nb;
    if (first + nb < count) e->sink.flag = nullptr;     // the last launch tells the host
    const unsigned * ps = scaler_ptr(e, parent_scaler_index), * cs = scaler_ptr(e, child_scaler_index);
    if (!f->derivatives(e, mv, params, tl, nb, d_sum, ps, cs, nblocks) ||
        !finish_launch(e, nblocks, e->blocked ? 8 : 2 * trial_instance(nb))) return PLL_FAILURE;
  }
  e->counters.derivative_calls++;
  e->counters.derivative_points += count;
  if (deferred) return PLL_SUCCESS;
  const volatile unsigned long long * flag =
      reinterpret_cast<const volatile unsigned long long *>(e->h_result) + RESULT_SEQ_SLOT;
  if (!wait_sequence(e->stream, flag, base.seq)) return PLL_FAILURE;
  for (unsigned i = 0; i < count; ++i) { out_df[i] = e->h_result[2 * i]; out_ddf[i] = e->h_result[2 * i + 1]; }
  if (asc)
    for (unsigned i = 0; i < count; ++i)
    {
      // d_f, dd_f are derivatives of -lnL: the correction's derivatives come off
      double d1, d2;
      asc_derivatives(p, e->h_asc + (size_t)i * e->S * 4, &d1, &d2);
      out_df[i] -= d1;
      out_ddf[i] -= d2;
    }
  return PLL_SUCCESS;
}

} // namespace pllhip

extern "C" {

double pll_compute_edge_loglikelihood(pll_partition_t * p,
                                      unsigned int parent_clv_index, int parent_scaler_index,
                                      unsigned int child_clv_index, int child_scaler_index,
                                      unsigned int matrix_index,
                                      const unsigned int * freqs_indices,
                                      double * persite_lnl)
{
  if (is_router(p))
    return router_loglikelihood(p, parent_clv_index, parent_scaler_index, child_clv_index,
                                child_scaler_index, (int)matrix_index, freqs_indices, persite_lnl);
  return loglikelihood_impl(p, parent_clv_index, parent_scaler_index, child_clv_index,
                            child_scaler_index, (int)matrix_index, freqs_indices, persite_lnl, nullptr);
}

double pll_compute_root_loglikelihood(pll_partition_t * p, unsigned int clv_index, int scaler_index,
                                      const unsigned int * freqs_indices, double * persite_lnl)
{
  if (is_router(p))
    return router_loglikelihood(p, clv_index, scaler_index, 0, PLL_SCALE_BUFFER_NONE, -1, freqs_indices, persite_lnl);
  return loglikelihood_impl(p, clv_index, scaler_index, 0, PLL_SCALE_BUFFER_NONE, -1,
                            freqs_indices, persite_lnl, nullptr);
}

int pll_update_sumtable(pll_partition_t * p,
                        unsigned int parent_clv_index, unsigned int child_clv_index,
                        int parent_scaler_index, int child_scaler_index,
                        const unsigned int * params_indices, double * sumtable)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    if (!ensure_eigen(p, params_indices)) return PLL_FAILURE;
    for (pll_partition_t * c : e->shards)
    {
      push_model(p, c);
      if (!pll_update_sumtable(c, parent_clv_index, child_clv_index, parent_scaler_index, child_scaler_index,
                               params_indices, sumtable))
        return PLL_FAILURE;
    }
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  if (!check_clv_index(e, parent_clv_index, "parent") || !check_clv_index(e, child_clv_index, "child") ||
      !check_scaler_index(e, parent_scaler_index) || !check_scaler_index(e, child_scaler_index))
    return PLL_FAILURE;
  if (!sumtable)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "sumtable key must not be NULL");
    return PLL_FAILURE;
  }
  if (!ensure_eigen(p, params_indices) || !sync_model(p)) return PLL_FAILURE;
  if (e->coded_tips && !ensure_luts(p)) return PLL_FAILURE;
  if (!need_clv(e, parent_clv_index) || !need_clv(e, child_clv_index)) return PLL_FAILURE;
  double * d_sum = sumtable_device(e, sumtable, true);
  if (!d_sum) return PLL_FAILURE;

  const ModelView mv = model_view(e);
  const ParamIdx params = make_params(p, params_indices);
  const NodeRef parent = node_ref(e, parent_clv_index), child = node_ref(e, child_clv_index);
  const int rc = edge_family(e)->sumtable(e, mv, params, parent, child, d_sum);
  e->counters.sumtable_calls++;
  return rc;
}

int pll_compute_likelihood_derivatives(pll_partition_t * p,
                                       int parent_scaler_index, int child_scaler_index,
                                       double branch_length,
                                       const unsigned int * params_indices,
                                       const double * sumtable, double * d_f, double * dd_f)
{
  if (is_router(p))
    return router_derivatives(p, parent_scaler_index, child_scaler_index, &branch_length, 1, params_indices,
                              sumtable, d_f, dd_f);
  return derivatives_impl(p, parent_scaler_index, child_scaler_index, &branch_length, 1, params_indices,
                          sumtable, nullptr, d_f, dd_f);
}

} // extern "C"

namespace pllhip {

// one partition's launch of the Newton-Raphson loop, everything resolved
struct NewtonLaunch
{
  Engine * e = nullptr;
  const void * fn = nullptr;
  size_t lds = 0;
  unsigned nblocks = 0;
  double share = 0.0;             // fraction of the chip its workgroups take while they are all resident
  double * d_sum = nullptr;
  const unsigned * ps = nullptr, * cs = nullptr;
  ModelView mv;
  ParamIdx params;
};

// checks and kernel choice of pllhip_newton_branch for one partition.  resident: the loop may keep the sumtable in the
// registers of one-workgroup-per-CU launches (a partition that has the device to itself); otherwise the streaming loop,
// whose workgroups leave room for the other partitions' launches.  Same grid either way: same block totals.
static int newton_prepare(pll_partition_t * p, int parent_scaler_index, int child_scaler_index,
                          const unsigned * params_indices, const double * sumtable, bool resident, NewtonLaunch & L)
{
  Engine * e = engine_of(p);
  static const int enabled = getenv("PLLHIP_DEVICE_NEWTON") ? atoi(getenv("PLLHIP_DEVICE_NEWTON")) : 1;
  const EdgeFamily * f = edge_family(e);
  const bool family_ok = f->newton_probe && (f->newton_rate_scalers || !e->rate_scalers);
  if (!enabled || !e->shards.empty() || !family_ok || e->N > e->Nreal || !e->fused_finish)
  {
    set_error(PLLHIP_ERROR_NEWTON_UNSUPPORTED, "this partition does not run the Newton-Raphson loop on the device");
    return PLL_FAILURE;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  if (!check_scaler_index(e, parent_scaler_index) || !check_scaler_index(e, child_scaler_index)) return PLL_FAILURE;
  L.e = e;
  L.d_sum = sumtable_device(e, sumtable, false);
  if (!L.d_sum)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_newton_branch: no sumtable was computed for this buffer");
    return PLL_FAILURE;
  }
  if (!sync_model(p) || !ensure_invariant(p)) return PLL_FAILURE;
  if (!need_scaler(e, parent_scaler_index) || !need_scaler(e, child_scaler_index)) return PLL_FAILURE;
  // the scan's own grid (derivatives_impl): the block totals, and with them every bit of the sums, are the same
  L.nblocks = scan_grid(e);
  int capacity = newton_capacity(e);
  if (capacity < 0) return PLL_FAILURE;
  L.fn = e->newton_fn;
  L.lds = e->newton_lds;
  if (!resident && e->newton_resident)
  {
    L.fn = e->newton_stream_fn;
    L.lds = e->newton_stream_lds;
    capacity = e->newton_stream_capacity;
  }
  // every workgroup waits for the others inside the launch: all of them have to be on the chip at once
  if ((int)L.nblocks > capacity || capacity == 0)
  {
    set_error(PLLHIP_ERROR_NEWTON_UNSUPPORTED, "the scan grid (%u workgroups) does not fit the chip at once (%d)",
              L.nblocks, capacity);
    return PLL_FAILURE;
  }
  L.share = (double)L.nblocks / (double)capacity;
  if (!e->d_newton)
  {
    if (!dev_alloc(reinterpret_cast<NewtonControl **>(&e->d_newton), 1, "Newton-Raphson control block")) return PLL_FAILURE;
    PLLHIP_TRY(hipMemsetAsync(e->d_newton, 0, sizeof(NewtonControl), e->stream));     // (`arrived`, `iter`: NewtonParams)
    PLLHIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_newton), 128 * sizeof(double), hipHostMallocMapped));
    memset(e->h_newton, 0, 128 * sizeof(double));
    PLLHIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&e->hd_newton), e->h_newton, 0));
  }
  L.mv = model_view(e);
  L.params = make_params(p, params_indices);
  L.ps = scaler_ptr(e, parent_scaler_index);
  L.cs = scaler_ptr(e, child_scaler_index);
  return PLL_SUCCESS;
}

// the launch: totals of the partition's scans go to its OWN control block's `tot`, everything else (iterate, bracket,
// status, trail, the partitions' meeting point) lives in `ctl`, results in host_out / host_flag
static int newton_launch(const NewtonLaunch & L, const NewtonParams & np_, NewtonControl * ctl, double * host_out,
                         unsigned long long * host_flag, unsigned long long seq)
{
  Engine * e = L.e;
  NewtonParams np = np_;
  ReduceOut ro;
  ro.block_out = e->d_partials;
  ro.counter = e->d_counter;
  ro.dst = static_cast<NewtonControl *>(e->d_newton)->tot;
  ro.flag = nullptr;
  ro.seq = 0;
  ro.fused = 1;
  ro.nq = 2;
  unsigned rs = e->rate_scalers ? 1u : 0u;
  if (!e->blocked)        // the 4-state loop: no site blocks and no per-rate scalers in its argument list
  {
    void * args4[] = {(void *)&L.mv, (void *)&L.params, (void *)&np, (void *)&L.d_sum, (void *)&L.ps, (void *)&L.cs,
                      (void *)&e->d_weights, (void *)&e->d_invariant, (void *)&e->N, (void *)&e->R,
                      (void *)&ro, (void *)&ctl, (void *)&host_out, (void *)&host_flag, (void *)&seq};
    PLLHIP_TRY(hipLaunchKernel(L.fn, dim3(L.nblocks), dim3(256), args4, 0, e->stream));
  }
  else
  {
    void * args[] = {(void *)&L.mv, (void *)&L.params, (void *)&np, (void *)&L.d_sum, (void *)&L.ps, (void *)&L.cs,
                     (void *)&e->d_weights, (void *)&e->d_invariant, (void *)&e->N, (void *)&e->nblk, (void *)&e->R,
                     (void *)&ro, (void *)&rs, (void *)&ctl, (void *)&host_out, (void *)&host_flag, (void *)&seq};
    PLLHIP_TRY(hipLaunchKernel(L.fn, dim3(L.nblocks), dim3(256), args, L.lds, e->stream));
  }
  e->counters.derivative_calls++;
  return PLL_SUCCESS;
}

static NewtonParams newton_params(double start, double bl_min, double bl_max, double tolerance, unsigned max_newton,
                                  unsigned nblocks_first)
{
  NewtonParams np;
  np.bl_min = bl_min; np.bl_max = bl_max; np.tolerance = tolerance;
  np.dxmax = bl_max / max_newton;
  np.max_newton = max_newton;
  np.x0 = std::max(std::min(start, bl_max), bl_min);
  // PLLHIP_NEWTON_SPIN_LIMIT: polls before a waiting workgroup gives up; PLLHIP_FAULT=newton_stall: workgroup 0 of
  // the next PLLHIP_FAULT_COUNT (default 1) launches never arrives (tests of the PLLHIP_ERROR_NEWTON_STUCK path)
  static const unsigned env_spin = getenv("PLLHIP_NEWTON_SPIN_LIMIT") ? (unsigned)strtoul(getenv("PLLHIP_NEWTON_SPIN_LIMIT"), nullptr, 10) : 0u;
  static std::atomic<int> stall_left{(getenv("PLLHIP_FAULT") && !strcmp(getenv("PLLHIP_FAULT"), "newton_stall"))
                                         ? (getenv("PLLHIP_FAULT_COUNT") ? atoi(getenv("PLLHIP_FAULT_COUNT")) : 1) : 0};
  np.spin_limit = env_spin ? env_spin : NEWTON_SPIN_LIMIT;
  np.stall_block = ~0u;
  // (launches of the process, whichever thread makes them: the count goes down once per stalled launch)
  if (nblocks_first > 1 && stall_left.load(std::memory_order_relaxed) > 0)
  {
    if (stall_left.fetch_sub(1, std::memory_order_relaxed) > 0) np.stall_block = 0u;
    else stall_left.fetch_add(1, std::memory_order_relaxed);
  }
  np.part = 0;
  np.nparts = 1;
  np.xscale = 1.0;
  np.debug = getenv("PLLHIP_NEWTON_DEBUG") ? 1u : 0u;
  np.iter_base = 0;
  return np;
}

static_assert(newton_range::MAX_NEWTON == PLLHIP_NEWTON_MAX_ITERATIONS, "include/pllhip.h documents the bound of max_newton");

// what the launches of one loop share: the control block in the lead partition's device memory, where the results go
struct NewtonRun { NewtonControl * ctl; double * host_out; unsigned long long * host_flag; unsigned long long seq; };

// Starts a loop on `lead`, on whose stream the caller has ordered everything that used the control block before.  The
// block is initialised from the kernel arguments -- NewtonParams::iter_base, the start of this loop's own range of
// `iter` values: the block's running counter (Engine::newton_iter) advances by the max_newton + 2 values the loop may
// publish, so no value it publishes or waits for is one an earlier loop can have left in the block, however many scans
// that loop made (newton_range.hpp; the entry points bound max_newton by newton_range::MAX_NEWTON) --;
// with PLLHIP_NEWTON_DEBUG the counters of the dump are reset by a copy (pageable source, staged by the runtime before
// the call returns).  nscales partitions with length_scalers (null: 1.0); 0: a loop of one partition, its scale in np.
static int newton_begin(Engine * lead, NewtonParams & np, const double * length_scalers, unsigned nscales, NewtonRun & run)
{
  run.ctl = static_cast<NewtonControl *>(lead->d_newton);
  run.seq = ++lead->newton_seq;
  np.iter_base = newton_range::take(lead->newton_iter, np.max_newton);
  if (np.debug)
  {
    NewtonControl init;
    memset(&init, 0, sizeof(init));
    init.x = np.x0; init.xl = np.bl_min; init.xh = np.bl_max; init.iter = 0; init.status = NEWTON_RUNNING;
    for (unsigned k = 0; k < nscales; ++k) init.pscale[k] = length_scalers ? length_scalers[k] : 1.0;
    PLLHIP_TRY(hipMemcpyAsync(run.ctl, &init, sizeof(init), hipMemcpyHostToDevice, lead->stream));
  }
  run.host_out = lead->hd_newton;
  run.host_flag = reinterpret_cast<unsigned long long *>(lead->hd_newton + 112);
  return PLL_SUCCESS;
}

// wait for the loop that `lead` hosts and translate how it ended; `all`: every engine that took part
static int newton_finish(Engine * lead, const std::vector<Engine *> & all, unsigned long long seq,
                         double * length, unsigned int * iterations, double * trail)
{
  const volatile unsigned long long * flag = reinterpret_cast<const volatile unsigned long long *>(lead->h_newton + 112);
  if (!wait_sequence(lead->stream, flag, seq)) return PLL_FAILURE;
  const unsigned its = (unsigned)lead->h_newton[1], status = (unsigned)lead->h_newton[2];
  if (status == NEWTON_STUCK)
  {
    // the grids drain by themselves (every wait is bounded); the tickets of the unfinished reductions go back to
    // zero before anything else uses them
    for (Engine * e : all)
    {
      PLLHIP_TRY(hipSetDevice(e->device));
      PLLHIP_TRY(hipStreamSynchronize(e->stream));
      if (getenv("PLLHIP_NEWTON_DEBUG"))
      {
        // where the loop stood: the meeting point and every instance's tickets
        NewtonControl c;
        std::vector<unsigned> t(REDUCE_COUNTER_WORDS);
        (void)hipMemcpy(&c, lead->d_newton, sizeof(c), hipMemcpyDeviceToHost);
        (void)hipMemcpy(t.data(), e->d_counter, t.size() * sizeof(unsigned), hipMemcpyDeviceToHost);
        fprintf(stderr, "newton stuck: instance %p iter %u status %u arrived %u x %g | tickets", (void *)e, c.iter, c.status, c.arrived, c.x);
        for (unsigned k = 0; k <= REDUCE_SHARDS; ++k) fprintf(stderr, " %u", t[k * REDUCE_SHARD_STRIDE]);
        fprintf(stderr, " | ptot");
        for (unsigned k = 0; k < all.size(); ++k) fprintf(stderr, " (%g %g)", c.ptot[k][0], c.ptot[k][1]);
        fprintf(stderr, " | waits entered / left / arrived-after-scan per instance:");
        for (unsigned k = 0; k < all.size(); ++k) fprintf(stderr, " %u/%u/%u", c.dbg_enter[k], c.dbg_leave[k], c.dbg_arrive[k]);
        fprintf(stderr, "\n");
      }
      PLLHIP_TRY(hipMemsetAsync(e->d_counter, 0, REDUCE_COUNTER_WORDS * sizeof(unsigned), e->stream));
      PLLHIP_TRY(hipStreamSynchronize(e->stream));
    }
    // ... and the meeting point of the partitions (`arrived`) with them: the next loop does not initialise it
    PLLHIP_TRY(hipSetDevice(lead->device));
    PLLHIP_TRY(hipMemsetAsync(lead->d_newton, 0, sizeof(NewtonControl), lead->stream));
    PLLHIP_TRY(hipStreamSynchronize(lead->stream));
    set_error(PLLHIP_ERROR_NEWTON_STUCK, "the device-resident Newton-Raphson loop did not get all its workgroups onto the "
              "chip at once (the device is shared with other work)");
    return PLL_FAILURE;
  }
  for (Engine * e : all) e->counters.derivative_points += its;
  if (length) *length = lead->h_newton[0];
  if (iterations) *iterations = its;
  if (trail) for (unsigned i = 0; i < its && i < NEWTON_TRAIL_MAX; ++i) trail[i] = lead->h_newton[NEWTON_TRAIL_SLOT + i];
  switch (status)
  {
    case NEWTON_CONVERGED: return PLL_SUCCESS;
    case NEWTON_LIMIT: set_error(PLLHIP_ERROR_NEWTON_LIMIT, "Exceeded maximum number of iterations"); return PLL_FAILURE;
    case NEWTON_NONFINITE: set_error(PLLHIP_ERROR_NEWTON_DERIVATIVES, "Wrong likelihood derivatives"); return PLL_FAILURE;
    default: set_error(PLL_ERROR_HIP_RUNTIME, "the device-resident Newton-Raphson loop did not complete (status %u)", status);
             return PLL_FAILURE;
  }
}

// device_job.hpp (the host arrays are local, hence the synchronise)
bool tip_pointer_tables(Engine * e, DevBuf<const double *> & clv, DevBuf<const uint8_t *> & codes)
{
  std::vector<const double *> h_clv(e->tips ? e->tips : 1, nullptr);
  std::vector<const uint8_t *> h_codes(e->tips ? e->tips : 1, nullptr);
  for (unsigned t = 0; t < e->tips; ++t) { h_clv[t] = e->d_clv[t]; h_codes[t] = e->coded_tips ? e->d_codes[t] : nullptr; }
  return clv.alloc(h_clv.size(), "tip table") && codes.alloc(h_codes.size(), "tip table") &&
         hip_ok(hipMemcpyAsync(clv.p, h_clv.data(), sizeof(void *) * h_clv.size(), hipMemcpyHostToDevice, e->stream),
                "upload tip table") &&
         hip_ok(hipMemcpyAsync(codes.p, h_codes.data(), sizeof(void *) * h_codes.size(), hipMemcpyHostToDevice, e->stream),
                "upload tip table") &&
         hip_ok(hipStreamSynchronize(e->stream), "upload tip table");
}

// device_job.hpp
bool matrix_tables(pll_partition_t * p, MatrixTables & out)
{
  if (is_router(p))
  {
    pll_partition_t * c = engine_of(p)->shards[0];
    push_model(p, c);
    p = c;
  }
  Engine * e = engine_of(p);
  if (!hip_ok(hipSetDevice(e->device), "hipSetDevice") || !sync_model(p) || !flush_pmatrices(p)) return false;
  out.pmat = e->d_pmat;
  out.model = e->d_model;
  out.off_weights = (unsigned)e->off_weights;
  out.off_pinv = (unsigned)e->off_pinv;
  out.off_freqs = (unsigned)e->off_freqs;
  return true;
}

static int sitecat_allow_lds()
{
#define PLLHIP_ATTR(KK) \
  PLLHIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sitecat_s16<KK>), hipFuncAttributeMaxDynamicSharedMemorySize, S16_MAX_LDS_BYTES))
  PLLHIP_ATTR(5); PLLHIP_ATTR(6); PLLHIP_ATTR(7); PLLHIP_ATTR(8);
#undef PLLHIP_ATTR
  return PLL_SUCCESS;
}

// device_job.hpp: the operand set-up of an edge reader (as anc_stage_add and loglikelihood_impl make it), then the
// family's table kernel on the engine's stream; nothing is waited for
// pm_other / lut_other: matrices [R][S][Sp] and lookup tables [R][codes][S] to use in place of those of `matrix_index`
// (the pair table's zeroed diagonal); null: the partition's own.  Such a pass writes its A planes alone: planes.B only
// says whether the case split has invariant terms, as in the pass before it
static bool sitecat_edge_table_with(pll_partition_t * p, unsigned parent_clv, int parent_scaler, unsigned child_clv,
                                    int child_scaler, unsigned matrix_index, const unsigned * freqs_indices,
                                    const SiteCatPlanes & planes, const double * pm_other, const double * lut_other)
{
  Engine * e = engine_of(p);
  if (!hip_ok(hipSetDevice(e->device), "hipSetDevice")) return false;
  if (!check_clv_index(e, parent_clv, "parent") || !check_clv_index(e, child_clv, "child") ||
      !check_scaler_index(e, parent_scaler) || !check_scaler_index(e, child_scaler)) return false;
  if (matrix_index >= e->nmat)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "matrix index out of range");
    return false;
  }
  if (!sync_model(p) || !flush_pmatrices(p) || !ensure_luts(p) || !ensure_invariant(p)) return false;
  const unsigned N = e->Nreal;
  if (!N) return true;
  if (!need_clv(e, parent_clv) || !need_clv(e, child_clv) || !need_scaler(e, parent_scaler) ||
      !need_scaler(e, child_scaler)) return false;
  const ModelView mv = model_view(e);
  const ParamIdx fidx = make_params(p, freqs_indices);
  const NodeRef parent = node_ref(e, parent_clv), child = node_ref(e, child_clv);
  const double * pm = pm_other ? pm_other : e->d_pmat + (size_t)matrix_index * e->R * e->S * e->Sp;
  const double * lut = !child.codes ? nullptr : pm_other ? lut_other : e->d_lut + (size_t)matrix_index * e->R * e->lut_codes * e->S;
  SiteCatSide sd;
  sd.ps = scaler_ptr(e, parent_scaler);
  sd.cs = scaler_ptr(e, child_scaler);
  sd.invariant = planes.B ? e->d_invariant : nullptr;
  sd.rate_scalers = e->rate_scalers ? 1u : 0u;
  SiteCatOut out;
  out.A = planes.A; out.B = pm_other ? nullptr : planes.B; out.c = pm_other ? nullptr : planes.c; out.plane = planes.plane;
  if (e->family == KernelFamily::S20 || e->family == KernelFamily::S16)
  {
    const unsigned nblk = (N + S20_BS - 1) / S20_BS;
    const unsigned grid = capped_grid("PLLHIP_SITECAT_BLOCKS", std::min((nblk + 3) / 4, e->cu_count * 8));
    if (e->family == KernelFamily::S20)
      hipLaunchKernelGGL(k_sitecat_s20, dim3(grid), dim3(256), sizeof(double) * e->R * s16_fr(5), e->stream,
                         mv, fidx, parent, child, pm, lut, e->lut_codes, e->d_tipmap, sd, N, nblk, e->R, out);
    else
    {
      if (sizeof(double) * e->R * s16_frags(e) > 64 * 1024 && !sitecat_allow_lds()) return false;
#define PLLHIP_CALL(KK) \
      hipLaunchKernelGGL(k_sitecat_s16<KK>, dim3(grid), dim3(256), sizeof(double) * e->R * s16_fr(KK), e->stream, \
                         mv, fidx, parent, child, pm, lut, e->lut_codes, e->d_tipmap, sd, N, nblk, e->R, out)
      PLLHIP_DISPATCH_KS(s16_ks(e), PLLHIP_CALL);
#undef PLLHIP_CALL
    }
  }
  else
  {
    // one thread per site; 4 states: per (site, rate)
    const size_t items = e->family == KernelFamily::S4 ? (size_t)N * e->R : N;
    const unsigned gx = capped_grid("PLLHIP_SITECAT_BLOCKS", grid_for(items, 256));
    if (e->family == KernelFamily::S4)
      hipLaunchKernelGGL(k_sitecat_s4, dim3(gx), dim3(256), 0, e->stream,
                         mv, fidx, parent, child, pm, lut, e->lut_codes, e->d_tipmap, sd, N, e->R, out);
    else
      hipLaunchKernelGGL(k_sitecat_generic, dim3(gx), dim3(256), 0, e->stream,
                         mv, fidx, parent, child, pm, lut, e->lut_codes, e->d_tipmap, e->rows, sd, N, e->R, out);
  }
  return hip_ok(hipGetLastError(), "site-category table kernel");
}

bool sitecat_edge_table(pll_partition_t * p, unsigned parent_clv, int parent_scaler, unsigned child_clv, int child_scaler,
                        unsigned matrix_index, const unsigned * freqs_indices, const SiteCatPlanes & planes)
{
  return sitecat_edge_table_with(p, parent_clv, parent_scaler, child_clv, child_scaler, matrix_index, freqs_indices, planes,
                                 nullptr, nullptr);
}

// ---- the joint sample of the ancestral states (device_job.hpp, kernels_ancsample.hpp) ----
bool ancsample_operands(pll_partition_t * p, const unsigned * freqs_indices, const unsigned * nodes, unsigned count,
                        AncsOperands & ops, AncsVector * views)
{
  Engine * e = engine_of(p);
  if (!hip_ok(hipSetDevice(e->device), "hipSetDevice")) return false;
  for (unsigned k = 0; k < count; ++k)
    if (!check_clv_index(e, nodes[k], "named")) return false;
  // (the order of sitecat_edge_table, which follows with the root edge)
  if (!sync_model(p) || !flush_pmatrices(p) || !ensure_luts(p) || !ensure_invariant(p)) return false;
  // vectors that exist as their operation only are stored by one list (children before parents), then the class tables
  // are expanded; storing writes the vector's own buffer alone, so a vector made valid stays valid for the others
  std::vector<unsigned> unstored;
  for (unsigned k = 0; k < count; ++k)
    if (e->ledger.live(nodes[k])) unstored.push_back(nodes[k]);
  if (!unstored.empty() && !e->transient_busy && !store_unstored(e, unstored)) return false;
  for (unsigned k = 0; k < count; ++k)
  {
    if (!need_clv(e, nodes[k])) return false;
    if (e->ledger.live(nodes[k]))
    {
      set_error(PLL_ERROR_PARAM_INVALID, "the vector of node %u exists as its operation only and cannot be stored beside "
                "the others", nodes[k]);
      return false;
    }
    const NodeRef ref = node_ref(e, nodes[k]);
    views[k].clv = ref.clv;
    views[k].codes = ref.codes;
  }
  const ModelView mv = model_view(e);
  ops.pmat = e->d_pmat;
  ops.weights = mv.base + mv.off_weights;
  ops.freqs = mv.base + mv.off_freqs;
  ops.fidx = make_params(p, freqs_indices);
  ops.invariant = e->d_invariant && e->invariant_uploaded ? e->d_invariant : nullptr;
  ops.tipmap = e->d_tipmap;
  ops.brows = e->rows;
  ops.R = e->R;
  ops.S = e->S;
  ops.Sp = e->Sp;
  ops.cu_count = e->cu_count;
  return true;
}

bool ancsample_walk(pll_partition_t * p, const AncsOperands & ops, const AncsLaunch & launch, unsigned grid)
{
  Engine * e = engine_of(p);
  const size_t lds = (size_t)launch.slots * ANCS_WG * sizeof(unsigned long long) + 256;
  hipLaunchKernelGGL(k_ancsample_walk, dim3(grid), dim3(ANCS_WG), lds, e->stream, ops, launch);
  return hip_ok(hipGetLastError(), "k_ancsample_walk");
}

// ---- the endpoint-pair table of an edge (device_job.hpp, kernels_substmap.hpp) ----
constexpr size_t SUBSTMAP_PARTIAL_BYTES = (size_t)32 << 20;      // the partial tiles of a call stay below this

static bool substmap_blocked(const Engine * e) { return e->family == KernelFamily::S20 || e->family == KernelFamily::S16; }

// sites a workgroup of the generic pair kernel stages at a time, and the slices of its tile
static unsigned substmap_chunk(const Engine * e) { return std::max(16u, std::min(256u, 1024u / e->S)); }
static unsigned substmap_slices(const Engine * e) { return std::max(1u, 256u / (e->S * e->S)); }

bool substmap_shape(pll_partition_t * p, const unsigned * freqs_indices, SubstmapShape & shape)
{
  Engine * e = engine_of(p);
  // (the order of sitecat_edge_table: the lookup tables, whose code count sizes lut0, follow the matrices)
  if (!hip_ok(hipSetDevice(e->device), "hipSetDevice") || !sync_model(p) || !flush_pmatrices(p) || !ensure_luts(p)) return false;
  const unsigned N = e->Nreal, nblk = (N + S20_BS - 1) / S20_BS;
  shape.plane = ((size_t)N + 1) & ~(size_t)1;
  shape.splane = (size_t)std::max(1u, nblk) * S20_BS;
  shape.pm_cells = (size_t)e->R * e->S * e->Sp;
  shape.lut_cells = lut_active(e) ? (size_t)e->R * e->lut_codes * e->S : 0;
  shape.pinv = false;
  for (unsigned r = 0; r < e->R; ++r) shape.pinv = shape.pinv || p->prop_invar[freqs_indices[r]] > 0.0;
  const unsigned long long work = substmap_blocked(e) ? (nblk + 3) / 4 : (N + substmap_chunk(e) - 1) / substmap_chunk(e);
  const unsigned long long fit = SUBSTMAP_PARTIAL_BYTES / (sizeof(double) * e->R * e->S * e->S);
  shape.grid = capped_grid("PLLHIP_SUBSTMAP_BLOCKS", std::min<unsigned long long>(std::min<unsigned long long>(work, (unsigned long long)e->cu_count * 4), std::max<unsigned long long>(1, fit)));
  return true;
}

bool substmap_scale(pll_partition_t * p, unsigned parent_clv, int parent_scaler, unsigned child_clv, int child_scaler,
                    unsigned matrix_index, const unsigned * freqs_indices, const SubstmapShape & shape,
                    const SubstmapBuffers & buf)
{
  Engine * e = engine_of(p);
  SiteCatPlanes planes;
  planes.A = buf.A; planes.B = buf.B; planes.c = buf.c; planes.plane = shape.plane;
  if (!sitecat_edge_table(p, parent_clv, parent_scaler, child_clv, child_scaler, matrix_index, freqs_indices, planes))
    return false;
  const unsigned N = e->Nreal;
  if (!hip_ok(hipMemsetAsync(buf.dropped, 0, sizeof(unsigned long long), e->stream), "memset")) return false;
  if (!N) return true;
  if (buf.A0)
  {
    // the same table under matrices whose diagonal is zero: the lookup tables of a coded child follow them
    const double * pm = e->d_pmat + (size_t)matrix_index * shape.pm_cells;
    hipLaunchKernelGGL(k_substmap_zero_diag, dim3(grid_for(shape.pm_cells, 256)), dim3(256), 0, e->stream, pm, buf.pm0, e->R,
                       e->S, e->Sp);
    if (shape.lut_cells)
      hipLaunchKernelGGL(k_rebuild_lut, dim3(1, e->R), dim3(256), 0, e->stream, e->S, e->Sp, e->R, buf.pm0, buf.lut0,
                         e->lut_codes, e->d_tipmap);
    if (!hip_ok(hipGetLastError(), "zeroed-diagonal matrices")) return false;
    planes.A = buf.A0;
    if (!sitecat_edge_table_with(p, parent_clv, parent_scaler, child_clv, child_scaler, matrix_index, freqs_indices, planes,
                                 buf.pm0, buf.lut0))
      return false;
  }
  SiteCatSide sd;
  sd.ps = scaler_ptr(e, parent_scaler);
  sd.cs = scaler_ptr(e, child_scaler);
  sd.invariant = buf.B ? e->d_invariant : nullptr;
  sd.rate_scalers = e->rate_scalers ? 1u : 0u;
  SubstScale io;
  io.A = buf.A; io.B = buf.B; io.A0 = buf.A0; io.plane = shape.plane; io.m = buf.m; io.scale = buf.scale;
  io.splane = shape.splane; io.differ = buf.differ; io.dropped = buf.dropped;
  hipLaunchKernelGGL(k_substmap_scale, dim3(capped_grid("PLLHIP_SUBSTMAP_BLOCKS", grid_for(shape.splane, 256))), dim3(256), 0,
                     e->stream, model_view(e), make_params(p, freqs_indices), sd, N, e->R, io);
  return hip_ok(hipGetLastError(), "pair-table scale kernel");
}

bool substmap_pairs(pll_partition_t * p, unsigned parent_clv, unsigned child_clv, const SubstmapShape & shape,
                    const SubstmapBuffers & buf)
{
  Engine * e = engine_of(p);
  const unsigned N = e->Nreal;
  if (!N) return hip_ok(hipMemsetAsync(buf.partial, 0, sizeof(double) * shape.grid * e->R * e->S * e->S, e->stream), "memset");
  const NodeRef parent = node_ref(e, parent_clv), child = node_ref(e, child_clv);
  if (substmap_blocked(e))
  {
    const unsigned nblk = (N + S20_BS - 1) / S20_BS;
#define PLLHIP_CALL(KK) \
    hipLaunchKernelGGL(k_substmap_pairs_blocked<KK>, dim3(shape.grid), dim3(256), 0, e->stream, parent, child, e->d_tipmap, \
                       buf.scale, shape.splane, N, nblk, e->R, e->S, buf.partial)
    PLLHIP_DISPATCH_KS(e->family == KernelFamily::S20 ? 5u : s16_ks(e), PLLHIP_CALL);
#undef PLLHIP_CALL
  }
  else
  {
    const unsigned CH = substmap_chunk(e), G = substmap_slices(e);
    const size_t lds = sizeof(double) * ((size_t)G * e->S * e->S + (size_t)2 * CH * e->S);
    hipLaunchKernelGGL(k_substmap_pairs_generic, dim3(shape.grid), dim3(256), lds, e->stream, parent, child, e->d_tipmap,
                       e->family == KernelFamily::S4 ? 0u : e->rows, buf.scale, shape.splane, N, e->R, e->S, e->Sp, CH, G,
                       buf.partial);
  }
  return hip_ok(hipGetLastError(), "pair-table kernel");
}

bool substmap_reduce(pll_partition_t * p, unsigned matrix_index, const unsigned * freqs_indices,
                     const SubstmapShape & shape, const SubstmapBuffers & buf)
{
  Engine * e = engine_of(p);
  const unsigned total = e->R * e->S * e->S;
  hipLaunchKernelGGL(k_substmap_reduce, dim3((total + 63) / 64), dim3(256), 0, e->stream, buf.partial, shape.grid, e->R, e->S,
                     e->Sp, e->d_pmat + (size_t)matrix_index * shape.pm_cells, model_view(e), make_params(p, freqs_indices),
                     buf.F, buf.pairs);
  return hip_ok(hipGetLastError(), "pair-table reduction");
}

} // namespace pllhip

extern "C" {

int pllhip_newton_branch(pll_partition_t * p, int parent_scaler_index, int child_scaler_index,
                         const unsigned int * params_indices, const double * sumtable,
                         double start, double bl_min, double bl_max, double tolerance, unsigned int max_newton,
                         double * length, unsigned int * iterations, double * trail)
{
  if (!newton_range::supported(max_newton))
  {
    set_error(PLLHIP_ERROR_NEWTON_UNSUPPORTED, "the device-resident Newton-Raphson loop takes an iteration limit of 1 to %u",
              (unsigned)newton_range::MAX_NEWTON);
    return PLL_FAILURE;
  }
  NewtonLaunch L;
  if (!newton_prepare(p, parent_scaler_index, child_scaler_index, params_indices, sumtable, true, L)) return PLL_FAILURE;
  Engine * e = L.e;
  NewtonParams np = newton_params(start, bl_min, bl_max, tolerance, max_newton, L.nblocks);
  NewtonRun run;
  if (!newton_begin(e, np, nullptr, 0, run)) return PLL_FAILURE;
  if (!newton_launch(L, np, run.ctl, run.host_out, run.host_flag, run.seq)) return PLL_FAILURE;
  return newton_finish(e, std::vector<Engine *>(1, e), run.seq, length, iterations, trail);
}

// The loop over several partitions runs one launch per partition, each on its partition's stream, and the launches wait
// for one another on the device: they have to be there TOGETHER.  Two streams that share a hardware queue run one after
// the other -- with five streams on the runtime's four queues the second instance started when the first had given up
// (PLLHIP_NEWTON_DEBUG=1 shows it) -- so the loop is offered only to a process that asked the runtime for enough queues
// before its first HIP call: GPU_MAX_HW_QUEUES >= 8 in the environment (the library does not set it: see
// pllhip_runtime_defaults for what it costs).  Elsewhere pllhip_newton_branch_multi answers
// PLLHIP_ERROR_NEWTON_UNSUPPORTED and the callers iterate from the host.
static bool newton_multi_enabled()
{
  static const bool on = []() { const char * q = getenv("GPU_MAX_HW_QUEUES"); return q && atoi(q) >= 8; }();
  return on;
}

// The loop over several partitions as ONE launch (k_newton_multi, kernels_newton_s4.hpp): every partition a run of the
// launch's workgroups.  -1: not for these partitions (a family without a place in the kernel, a 4-state partition whose
// table does not fit the registers, grids that do not fit the chip together): the caller tries the other forms.
static int newton_multi_one_launch(pll_partition_t * const * partitions, unsigned count, int parent_scaler_index,
                                   int child_scaler_index, const unsigned int * const * params_indices,
                                   const double * const * sumtables, const double * length_scalers,
                                   double start, double bl_min, double bl_max, double tolerance, unsigned max_newton,
                                   double * length, unsigned * iterations, double * trail)
{
  static const int enabled = getenv("PLLHIP_NEWTON_ONE_LAUNCH") ? atoi(getenv("PLLHIP_NEWTON_ONE_LAUNCH")) : 1;
  if (!enabled) return -1;
  for (unsigned k = 0; k < count; ++k)
    if (!edge_family(engine_of(partitions[k]))->newton_kind) return -1;
  std::vector<NewtonLaunch> L(count);
  NewtonMultiArgs args;
  memset(&args, 0, sizeof(args));
  unsigned total = 0;
  size_t lds = 0;
  const int saved_errno = pll_errno;
  for (unsigned k = 0; k < count; ++k)
  {
    // (the streaming form of the matrix-core families: the sumtable of a slice fits the registers of a launch of its
    // own, not of a shared one)
    if (!newton_prepare(partitions[k], parent_scaler_index, child_scaler_index, params_indices[k], sumtables[k], false, L[k]))
    {
      if (pll_errno != PLLHIP_ERROR_NEWTON_UNSUPPORTED) return PLL_FAILURE;
      pll_errno = saved_errno;
      return -1;
    }
    Engine * e = L[k].e;
    NewtonMultiPart & P = args.part[k];
    P.mv = L[k].mv; P.params = L[k].params; P.sumtable = L[k].d_sum; P.ps = L[k].ps; P.cs = L[k].cs;
    P.weights = e->d_weights; P.invariant = e->d_invariant;
    P.ro.block_out = e->d_partials; P.ro.counter = e->d_counter; P.ro.dst = static_cast<NewtonControl *>(e->d_newton)->tot;
    P.ro.flag = nullptr; P.ro.seq = 0; P.ro.fused = 1; P.ro.nq = 2;
    P.xscale = length_scalers ? length_scalers[k] : 1.0;
    P.N = e->N; P.nblk = e->nblk; P.R = e->R; P.rate_scalers = e->rate_scalers ? 1u : 0u;
    P.kind = edge_family(e)->newton_kind(e);
    P.first_block = total; P.nblocks = L[k].nblocks;
    total += L[k].nblocks;
    lds = std::max(lds, newton_table_lds(e, edge_family(e)->newton_ks(e)));
  }
  Engine * lead = L[0].e;
  PLLHIP_TRY(hipSetDevice(lead->device));
  if (lds > 64 * 1024) return -1;
  // every workgroup waits for the others inside the launch: all of them on the chip at once
  bool any16 = false;
  for (unsigned k = 0; k < count; ++k) any16 = any16 || args.part[k].kind >= NEWTON_KIND_S16;
  const void * fn = any16 ? reinterpret_cast<const void *>(k_newton_multi<true>) : reinterpret_cast<const void *>(k_newton_multi<false>);
  int & per_cu = lead->newton_multi_per_cu[any16 ? 1 : 0][lds > 16 * 1024 ? 1 : 0];
  if (per_cu < 0 &&
      !hip_ok(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256,
                                                          lds > 16 * 1024 ? 64 * 1024 : 16 * 1024), "hipOccupancyMaxActiveBlocksPerMultiprocessor"))
    return PLL_FAILURE;
  // (one launch: the dispatcher fills the chip with its workgroups alone, so all of what the chip holds may be asked for
  // -- as in the loop of a single partition)
  if (per_cu <= 0 || total > (unsigned)per_cu * lead->cu_count) return -1;
  args.np = newton_params(start, bl_min, bl_max, tolerance, max_newton, L[0].nblocks);
  args.np.nparts = count;
  args.nparts = count;
  // the launch runs on the first partition's stream: after what the others have issued (their sumtables) ...
  for (unsigned k = 1; k < count; ++k)
  {
    Engine * e = L[k].e;
    if (e->stream == lead->stream) continue;
    if (!e->newton_ready) PLLHIP_TRY(hipEventCreateWithFlags(&e->newton_ready, hipEventDisableTiming));
    PLLHIP_TRY(hipEventRecord(e->newton_ready, e->stream));
    PLLHIP_TRY(hipStreamWaitEvent(lead->stream, e->newton_ready, 0));
    // (... and after the instance of an earlier loop of the other form, should there have been one)
    if (e->newton_done) PLLHIP_TRY(hipStreamWaitEvent(lead->stream, e->newton_done, 0));
  }
  NewtonRun run;
  if (!newton_begin(lead, args.np, length_scalers, count, run)) return PLL_FAILURE;
  void * kargs[] = {(void *)&args, (void *)&run.ctl, (void *)&run.host_out, (void *)&run.host_flag, (void *)&run.seq};
  PLLHIP_TRY(hipLaunchKernel(fn, dim3(total), dim3(256), kargs, lds, lead->stream));
  std::vector<Engine *> all;
  for (unsigned k = 0; k < count; ++k) { all.push_back(L[k].e); L[k].e->counters.derivative_calls++; }
  // ... and what the others issue next comes after it
  if (!lead->newton_done) PLLHIP_TRY(hipEventCreateWithFlags(&lead->newton_done, hipEventDisableTiming));
  PLLHIP_TRY(hipEventRecord(lead->newton_done, lead->stream));
  for (unsigned k = 1; k < count; ++k)
    if (L[k].e->stream != lead->stream) PLLHIP_TRY(hipStreamWaitEvent(L[k].e->stream, lead->newton_done, 0));
  return newton_finish(lead, all, run.seq, length, iterations, trail);
}

// Several partitions under ONE branch length (linked lengths, or scaled ones: partition p sees s_p x): the loop of
// pllhip_newton_branch with the sum over the partitions inside it.  Every partition launches its own instance of the
// loop on its own stream -- its family's kernel on its own scan grid, so its totals are the ones its blocking derivative
// call returns, bit for bit --; the instances meet in the first partition's control block after every scan (the
// partition that arrives last adds the totals in partition order and applies the step rule) and all wait there for the
// next iterate.  All launches have to be resident together: their shares of the chip must add up to less than one
// (with the register-resident form where that fits, else the streaming form), otherwise PLLHIP_ERROR_NEWTON_UNSUPPORTED.
int pllhip_newton_branch_multi(pll_partition_t * const * partitions, unsigned int count,
                               int parent_scaler_index, int child_scaler_index,
                               const unsigned int * const * params_indices, const double * const * sumtables,
                               const double * length_scalers,
                               double start, double bl_min, double bl_max, double tolerance, unsigned int max_newton,
                               double * length, unsigned int * iterations, double * trail)
{
  if (count == 1 && (!length_scalers || length_scalers[0] == 1.0))
    return pllhip_newton_branch(partitions[0], parent_scaler_index, child_scaler_index, params_indices[0], sumtables[0],
                                start, bl_min, bl_max, tolerance, max_newton, length, iterations, trail);
  if (!count || count > NEWTON_MAX_PARTS || !newton_range::supported(max_newton))
  {
    set_error(PLLHIP_ERROR_NEWTON_UNSUPPORTED, "1 to %u partitions and an iteration limit of 1 to %u per device-resident "
              "Newton-Raphson loop", NEWTON_MAX_PARTS, (unsigned)newton_range::MAX_NEWTON);
    return PLL_FAILURE;
  }
  for (unsigned k = 0; k < count; ++k)
    if (!partitions[k] || engine_of(partitions[k])->device != engine_of(partitions[0])->device)
    {
      set_error(PLLHIP_ERROR_NEWTON_UNSUPPORTED, "the partitions of a device-resident Newton-Raphson loop live on one device");
      return PLL_FAILURE;
    }
  // all partitions in ONE launch where their families have a place in it (4, 20, 33 .. 64 states): no hardware queue
  // per partition needed
  {
    const int rc = newton_multi_one_launch(partitions, count, parent_scaler_index, child_scaler_index, params_indices, sumtables,
                                           length_scalers, start, bl_min, bl_max, tolerance, max_newton, length, iterations, trail);
    if (rc >= 0) return rc;
  }
  if (!newton_multi_enabled())
  {
    set_error(PLLHIP_ERROR_NEWTON_UNSUPPORTED, "the Newton-Raphson loop over these partitions runs as one launch per partition and "
              "needs a hardware queue per partition stream: GPU_MAX_HW_QUEUES >= 8 in the environment before the first HIP call");
    return PLL_FAILURE;
  }
  // (a launch's share = its workgroups / the workgroups of its kernel the chip holds: an upper bound of the resources
  // it takes, so shares that add up to one fit; the margin is for the order in which the dispatcher fills the CUs.
  // A wrong guess costs one bounded wait: PLLHIP_ERROR_NEWTON_STUCK, and the caller's own loop from then on)
  static const double max_share = getenv("PLLHIP_NEWTON_MAX_SHARE") ? atof(getenv("PLLHIP_NEWTON_MAX_SHARE")) : 0.9;
  std::vector<NewtonLaunch> L(count);
  bool fits = false;
  for (int resident = 1; resident >= 0 && !fits; --resident)
  {
    double share = 0.0;
    for (unsigned k = 0; k < count; ++k)
    {
      L[k] = NewtonLaunch();
      if (!newton_prepare(partitions[k], parent_scaler_index, child_scaler_index, params_indices[k], sumtables[k],
                          resident != 0, L[k]))
        return PLL_FAILURE;
      share += L[k].share;
    }
    fits = share <= max_share + 1e-9;
  }
  if (!fits)
  {
    set_error(PLLHIP_ERROR_NEWTON_UNSUPPORTED, "the scan grids of the %u partitions do not fit the chip together", count);
    return PLL_FAILURE;
  }
  Engine * lead = L[0].e;
  NewtonParams np = newton_params(start, bl_min, bl_max, tolerance, max_newton, L[0].nblocks);
  PLLHIP_TRY(hipSetDevice(lead->device));
  // (the instances are different kernels on different hardware queues -- pllhip_runtime_defaults asks the runtime for
  // enough of them; they meet in the first partition's control block, after the instances of the previous loop of
  // these partitions have left the device: they read the block to the end)
  for (unsigned k = 1; k < count; ++k)
    if (L[k].e->newton_done) PLLHIP_TRY(hipStreamWaitEvent(lead->stream, L[k].e->newton_done, 0));
  NewtonRun run;
  if (!newton_begin(lead, np, length_scalers, count, run)) return PLL_FAILURE;
  // the other partitions' launches use the control block: after the instances of the previous loop have left it
  if (!lead->newton_ready) PLLHIP_TRY(hipEventCreateWithFlags(&lead->newton_ready, hipEventDisableTiming));
  PLLHIP_TRY(hipEventRecord(lead->newton_ready, lead->stream));
  std::vector<Engine *> all;
  np.nparts = count;
  // (an instance that shares a hardware queue with another one never meets it: a shorter bound than the single loop's)
  static const bool env_spin_set = getenv("PLLHIP_NEWTON_SPIN_LIMIT") != nullptr;
  if (!env_spin_set) np.spin_limit = NEWTON_SPIN_LIMIT >> 4;
  for (unsigned k = 0; k < count; ++k)
  {
    np.part = k;
    np.xscale = length_scalers ? length_scalers[k] : 1.0;
    if (k) { np.stall_block = ~0u; PLLHIP_TRY(hipStreamWaitEvent(L[k].e->stream, lead->newton_ready, 0)); }
    all.push_back(L[k].e);
    if (!newton_launch(L[k], np, run.ctl, run.host_out, run.host_flag, run.seq))
    {
      // (the instances already launched give up after their bounded wait)
      (void)newton_finish(lead, all, run.seq, nullptr, nullptr, nullptr);
      return PLL_FAILURE;
    }
    if (k)
    {
      if (!L[k].e->newton_done) PLLHIP_TRY(hipEventCreateWithFlags(&L[k].e->newton_done, hipEventDisableTiming));
      PLLHIP_TRY(hipEventRecord(L[k].e->newton_done, L[k].e->stream));
    }
  }
  return newton_finish(lead, all, run.seq, length, iterations, trail);
}

unsigned int pllhip_free_trial_lengths(const pll_partition_t * p)
{
  return exec_engine(p)->blocked ? 4u : 1u;
}

int pllhip_set_sharding(unsigned int count, const int * devices)
{
  g_shard_devices.clear();
  g_shard_devices_set = true;
  if (count <= 1) return PLL_SUCCESS;
  const int n = pllhip_device_count();
  if (n < 1)
  {
    set_error(PLL_ERROR_HIP_NODEVICE, "No HIP device available");
    return PLL_FAILURE;
  }
  for (unsigned k = 0; k < count; ++k) g_shard_devices.push_back(devices ? devices[k] : (int)(k % (unsigned)n));
  return PLL_SUCCESS;
}

unsigned int pllhip_shard_count(const pll_partition_t * p)
{
  return is_router(p) ? (unsigned)engine_of(p)->shards.size() : 1u;
}

int pllhip_compute_likelihood_derivatives_multi(pll_partition_t * p,
                                                int parent_scaler_index, int child_scaler_index,
                                                const double * branch_lengths, unsigned int count,
                                                const unsigned int * params_indices,
                                                const double * sumtable, double * d_f, double * dd_f)
{
  if (is_router(p))
  {
    if (!count || count > MAX_TRIAL_LENGTHS)
    {
      set_error(PLL_ERROR_PARAM_INVALID, "1 to %u trial branch lengths per call", MAX_TRIAL_LENGTHS);
      return PLL_FAILURE;
    }
    return router_derivatives(p, parent_scaler_index, child_scaler_index, branch_lengths, count, params_indices,
                              sumtable, d_f, dd_f);
  }
  return derivatives_impl(p, parent_scaler_index, child_scaler_index, branch_lengths, count, params_indices,
                          sumtable, nullptr, d_f, dd_f);
}

int pll_update_invariant_sites(pll_partition_t * p)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    if (!p->invariant) p->invariant = static_cast<int *>(malloc(sizeof(int) * (p->sites ? p->sites : 1)));
    if (!p->invariant) { set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate invariant sites array"); return PLL_FAILURE; }
    for (size_t k = 0; k < e->shards.size(); ++k)
    {
      if (!pll_update_invariant_sites(e->shards[k])) return PLL_FAILURE;
      memcpy(p->invariant + e->shard_first[k], e->shards[k]->invariant, sizeof(int) * e->shards[k]->sites);
    }
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  if (!upload_tipmap(p)) return PLL_FAILURE;
  if (!p->invariant)
    p->invariant = static_cast<int *>(malloc(sizeof(int) * (e->N ? e->N : 1)));
  if (!p->invariant)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate invariant sites array");
    return PLL_FAILURE;
  }
  if (!e->d_invariant)
    if (!dev_alloc(&e->d_invariant, (size_t)e->N, "invariant sites")) return PLL_FAILURE;
  DevBuf<const double *> d_tc;
  DevBuf<const uint8_t *> d_tk;
  if (!tip_pointer_tables(e, d_tc, d_tk)) return PLL_FAILURE;
  hipLaunchKernelGGL(k_invariant, dim3(reduce_grid(e)), dim3(256), 0, e->stream,
                     d_tc.p, d_tk.p, e->d_tipmap, e->tips, e->N, e->R, e->S, e->Sp, e->rows, e->d_invariant);
  PLLHIP_TRY(hipGetLastError());
  if (e->N)
    PLLHIP_TRY(hipMemcpyAsync(p->invariant, e->d_invariant, sizeof(int) * e->N, hipMemcpyDeviceToHost, e->stream));
  PLLHIP_TRY(hipStreamSynchronize(e->stream));
  e->invariant_uploaded = true;
  return PLL_SUCCESS;
}

int pll_compute_node_ancestral(pll_partition_t * p, unsigned int node_clv_index, int node_scaler_index,
                               unsigned int other_clv_index, int other_scaler_index,
                               unsigned int matrix_index, const unsigned int * freqs_indices,
                               double * ancestral)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    for (size_t k = 0; k < e->shards.size(); ++k)
    {
      push_model(p, e->shards[k]);
      if (!pll_compute_node_ancestral(e->shards[k], node_clv_index, node_scaler_index, other_clv_index,
                                      other_scaler_index, matrix_index, freqs_indices,
                                      ancestral + (size_t)e->shard_first[k] * e->S))
        return PLL_FAILURE;
    }
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  if (!check_clv_index(e, node_clv_index, "node") || !check_clv_index(e, other_clv_index, "other") ||
      !check_scaler_index(e, node_scaler_index) || !check_scaler_index(e, other_scaler_index))
    return PLL_FAILURE;
  if (matrix_index >= e->nmat)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "matrix index out of range");
    return PLL_FAILURE;
  }
  if (!sync_model(p) || !flush_pmatrices(p) || !ensure_luts(p)) return PLL_FAILURE;
  if (!e->N) return PLL_SUCCESS;
  if (!need_clv(e, node_clv_index) || !need_clv(e, other_clv_index)) return PLL_FAILURE;
  // the result is normalised per site, so scaler counts cancel
  DevBuf<double> d_out;
  if (!d_out.alloc((size_t)e->N * e->S, "ancestral states")) return PLL_FAILURE;
  const unsigned gx = (unsigned)std::min<unsigned long long>(((unsigned long long)e->N + 255) / 256, 4096);
  hipLaunchKernelGGL(k_node_ancestral, dim3(gx), dim3(256), 0, e->stream,
                     model_view(e), make_params(p, freqs_indices), node_ref(e, node_clv_index),
                     node_ref(e, other_clv_index),
                     e->d_pmat + (size_t)matrix_index * e->R * e->S * e->Sp, e->d_tipmap, e->rows,
                     e->N, e->R, d_out.p);
  PLLHIP_TRY(hipGetLastError());
  PLLHIP_TRY(hipMemcpyAsync(ancestral, d_out.p, sizeof(double) * e->N * e->S, hipMemcpyDeviceToHost, e->stream));
  PLLHIP_TRY(hipStreamSynchronize(e->stream));
  return PLL_SUCCESS;
}

}   // extern "C"

namespace pllhip {

// ---------------------------------------------------------------------------
// pllhip_node_ancestral_begin / _add / _finish / _batch: marginal ancestral states of many nodes with the results
// staged on the device (kernels_ancestral.hpp).  An entry's kernel writes its summary (and, with PLLHIP_ANC_PROBS,
// its table) into a slot of one staging buffer per device, allocated once per batch; the host copies are enqueued
// and waited for once per staging chunk.  A slot is written in stream order, so the vectors of an entry may be
// overwritten by whatever the caller enqueues next.
// ---------------------------------------------------------------------------
struct AncPending { unsigned slot; unsigned char * states; double * state_probs; double * probs; };

struct AncStage                       // one device's part of a batch: an ordinary partition, or a shard
{
  pll_partition_t * p = nullptr;
  size_t first = 0;                   // first site of this part in the caller's arrays
  unsigned char * d_buf = nullptr;
  size_t off_probs_state = 0, off_probs = 0, entry_bytes = 0;
  unsigned cap = 0;
  bool table = false;                 // the slot holds a sites x states table (asked for, or the family needs it)
  std::vector<AncPending> pending;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  double kernel_ms = 0.0;             // between the events of the entries delivered so far
  unsigned long long chunks = 0;
};

}   // namespace pllhip

struct pllhip_anc_batch
{
  pll_partition_t * p;
  unsigned flags;
  bool failed;
  std::vector<pllhip::AncStage> stages;
};

namespace pllhip {

static thread_local double g_anc_kernel_ms = 0.0;
static thread_local unsigned long long g_anc_chunks = 0;

static size_t anc_align(size_t v) { return (v + 255) & ~(size_t)255; }

static size_t anc_budget()
{
  const char * env = getenv("PLLHIP_ANC_STAGING_BYTES");
  const long long v = env ? atoll(env) : 0;
  return v > 0 ? (size_t)v : (size_t)1 << 30;
}

// PLLHIP_ANC_BLOCKS: a cap on the workgroups of every ancestral-state launch (0 or unset: none), read at every call.
// For tests: with a small cap a wave walks many site blocks, which the default grid asks for only above ~260 000 sites.
static unsigned anc_grid(unsigned long long wanted)
{
  const char * env = getenv("PLLHIP_ANC_BLOCKS");
  const long long cap = env ? atoll(env) : 0;
  if (cap > 0 && (unsigned long long)cap < wanted) wanted = (unsigned long long)cap;
  return (unsigned)std::max<unsigned long long>(1, wanted);
}

static bool anc_family_fused(const Engine * e)
{
  return e->family == KernelFamily::S4 || e->family == KernelFamily::S20 || e->family == KernelFamily::S16;
}

static int anc_stage_init(AncStage & st, pll_partition_t * p, size_t first, unsigned flags, unsigned expected)
{
  Engine * e = engine_of(p);
  st.p = p;
  st.first = first;
  st.table = (flags & PLLHIP_ANC_PROBS) || !anc_family_fused(e);
  const size_t n = e->Nreal;
  st.off_probs_state = anc_align(n);
  st.off_probs = st.off_probs_state + anc_align(n * sizeof(double));
  st.entry_bytes = st.off_probs + (st.table ? anc_align(n * e->S * sizeof(double)) : 0);
  // (an entry is the unit: a budget below one entry still stages one)
  const size_t fit = std::max<size_t>(1, anc_budget() / st.entry_bytes);
  st.cap = (unsigned)std::min<size_t>(fit, expected ? expected : 0xffffffffu);
  if (!n) return PLL_SUCCESS;
  PLLHIP_TRY(hipSetDevice(e->device));
  return dev_alloc(&st.d_buf, st.entry_bytes * st.cap, "ancestral-state staging") ? PLL_SUCCESS : PLL_FAILURE;
}

// copies of every staged entry to the caller's arrays, one wait
static int anc_stage_flush(AncStage & st, unsigned flags)
{
  if (st.pending.empty()) return PLL_SUCCESS;
  Engine * e = engine_of(st.p);
  const size_t n = e->Nreal;
  PLLHIP_TRY(hipSetDevice(e->device));
  for (const AncPending & pd : st.pending)
  {
    const unsigned char * slot = st.d_buf + st.entry_bytes * pd.slot;
    PLLHIP_TRY(hipMemcpyAsync(pd.states + st.first, slot, n, hipMemcpyDeviceToHost, e->stream));
    PLLHIP_TRY(hipMemcpyAsync(pd.state_probs + st.first, slot + st.off_probs_state, n * sizeof(double),
                              hipMemcpyDeviceToHost, e->stream));
    if (flags & PLLHIP_ANC_PROBS)
      PLLHIP_TRY(hipMemcpyAsync(pd.probs + st.first * e->S, slot + st.off_probs, n * e->S * sizeof(double),
                                hipMemcpyDeviceToHost, e->stream));
  }
  const size_t staged = st.pending.size();
  st.pending.clear();
  PLLHIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t k = 0; k < staged && k < st.events.size(); ++k)
  {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, st.events[k].first, st.events[k].second) == hipSuccess) st.kernel_ms += ms;
  }
  st.chunks++;
  return PLL_SUCCESS;
}

static int anc_allow_lds()
{
#define PLLHIP_ATTR(KK) \
  PLLHIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_anc_s16<KK>), hipFuncAttributeMaxDynamicSharedMemorySize, S16_MAX_LDS_BYTES))
  PLLHIP_ATTR(5); PLLHIP_ATTR(6); PLLHIP_ATTR(7); PLLHIP_ATTR(8);
#undef PLLHIP_ATTR
  return PLL_SUCCESS;
}

static int anc_stage_add(AncStage & st, unsigned flags, unsigned node_clv_index, unsigned other_clv_index,
                         unsigned matrix_index, const unsigned * freqs_indices, unsigned char * states,
                         double * state_probs, double * probs)
{
  pll_partition_t * p = st.p;
  Engine * e = engine_of(p);
  PLLHIP_TRY(hipSetDevice(e->device));
  if (!check_clv_index(e, node_clv_index, "node") || !check_clv_index(e, other_clv_index, "other")) return PLL_FAILURE;
  if (matrix_index >= e->nmat)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "matrix index out of range");
    return PLL_FAILURE;
  }
  if (!sync_model(p) || !flush_pmatrices(p) || !ensure_luts(p)) return PLL_FAILURE;
  const unsigned N = e->Nreal;
  if (!N) return PLL_SUCCESS;
  if (!need_clv(e, node_clv_index) || !need_clv(e, other_clv_index)) return PLL_FAILURE;
  if (st.pending.size() == st.cap && !anc_stage_flush(st, flags)) return PLL_FAILURE;
  const unsigned slot = (unsigned)st.pending.size();
  unsigned char * base = st.d_buf + st.entry_bytes * slot;
  AncOut out;
  out.states = base;
  out.state_probs = reinterpret_cast<double *>(base + st.off_probs_state);
  out.probs = st.table ? reinterpret_cast<double *>(base + st.off_probs) : nullptr;

  const ModelView mv = model_view(e);
  const ParamIdx fidx = make_params(p, freqs_indices);
  const NodeRef node = node_ref(e, node_clv_index), other = node_ref(e, other_clv_index);
  const double * pm = e->d_pmat + (size_t)matrix_index * e->R * e->S * e->Sp;
  const double * lut = other.codes ? e->d_lut + (size_t)matrix_index * e->R * e->lut_codes * e->S : nullptr;
  if (st.events.size() <= slot)
  {
    std::pair<hipEvent_t, hipEvent_t> ev;
    PLLHIP_TRY(hipEventCreate(&ev.first));
    if (hipEventCreate(&ev.second) != hipSuccess) { (void)hipEventDestroy(ev.first); set_error(PLL_ERROR_HIP_RUNTIME, "hipEventCreate"); return PLL_FAILURE; }
    st.events.push_back(ev);
  }
  PLLHIP_TRY(hipEventRecord(st.events[slot].first, e->stream));
  if (e->family == KernelFamily::S20 || e->family == KernelFamily::S16)
  {
    const unsigned nblk = (N + S20_BS - 1) / S20_BS;
    const unsigned grid = anc_grid(std::min((nblk + 3) / 4, e->cu_count * 8));
    const bool tbl = out.probs != nullptr;
    if (e->family == KernelFamily::S20)
      hipLaunchKernelGGL(k_anc_s20, dim3(grid), dim3(256), sizeof(double) * anc_blocked_lds<5>(e->R, e->S, tbl), e->stream,
                         mv, fidx, node, other, pm, lut, e->lut_codes, e->d_tipmap, N, nblk, e->R, out);
    else
    {
      const unsigned ks = s16_ks(e);
      if (sizeof(double) * (e->R * s16_frags(e) + 4 * S20_BS * anc_tile_stride(e->S)) > 64 * 1024 && !anc_allow_lds())
        return PLL_FAILURE;
#define PLLHIP_CALL(KK) \
      hipLaunchKernelGGL(k_anc_s16<KK>, dim3(grid), dim3(256), sizeof(double) * anc_blocked_lds<KK>(e->R, e->S, tbl), e->stream, \
                         mv, fidx, node, other, pm, lut, e->lut_codes, e->d_tipmap, N, nblk, e->R, out)
      PLLHIP_DISPATCH_KS(ks, PLLHIP_CALL);
#undef PLLHIP_CALL
    }
  }
  else
  {
    const unsigned gx = anc_grid(std::min<unsigned long long>(((unsigned long long)N + 255) / 256, 4096));
    if (e->family == KernelFamily::S4)
      hipLaunchKernelGGL(k_anc_s4, dim3(gx), dim3(256), 0, e->stream,
                         mv, fidx, node, other, pm, lut, e->lut_codes, e->d_tipmap, N, e->R, out);
    else
    {
      hipLaunchKernelGGL(k_anc_generic, dim3(gx), dim3(256), 0, e->stream,
                         mv, fidx, node, other, pm, e->d_tipmap, e->rows, N, e->R, out.probs);
      PLLHIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_anc_summary, dim3(gx), dim3(256), 0, e->stream,
                         out.probs, N, e->S, out.states, out.state_probs);
    }
  }
  PLLHIP_TRY(hipGetLastError());
  PLLHIP_TRY(hipEventRecord(st.events[slot].second, e->stream));
  st.pending.push_back(AncPending{slot, states, state_probs, probs});
  return PLL_SUCCESS;
}

static void anc_stage_release(AncStage & st)
{
  if (!st.p) return;
  (void)hipSetDevice(engine_of(st.p)->device);
  for (auto & ev : st.events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
  st.events.clear();
  if (st.d_buf) (void)hipFree(st.d_buf);
  st.d_buf = nullptr;
}

}   // namespace pllhip

extern "C" {

pllhip_anc_batch_t * pllhip_node_ancestral_begin(pll_partition_t * p, unsigned int flags, unsigned int expected)
{
  if (!p || (flags & ~PLLHIP_ANC_PROBS))
  {
    set_error(PLL_ERROR_PARAM_INVALID, "ancestral states: no partition, or unknown flags");
    return nullptr;
  }
  if (p->states > 256)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "ancestral states: more than 256 states do not fit the state array");
    return nullptr;
  }
  Engine * e = engine_of(p);
  pllhip_anc_batch_t * b = new pllhip_anc_batch;
  b->p = p;
  b->flags = flags;
  b->failed = false;
  const size_t parts = e->shards.empty() ? 1 : e->shards.size();
  b->stages.resize(parts);
  for (size_t k = 0; k < parts; ++k)
    if (!anc_stage_init(b->stages[k], e->shards.empty() ? p : e->shards[k], e->shards.empty() ? 0 : e->shard_first[k],
                        flags, expected))
    {
      for (AncStage & st : b->stages) anc_stage_release(st);
      delete b;
      return nullptr;
    }
  return b;
}

int pllhip_node_ancestral_add(pllhip_anc_batch_t * b, unsigned int node_clv_index, unsigned int other_clv_index,
                              unsigned int matrix_index, const unsigned int * freqs_indices,
                              unsigned char * states, double * state_probs, double * probs)
{
  if (!b || !states || !state_probs || !freqs_indices || ((b->flags & PLLHIP_ANC_PROBS) && !probs))
  {
    set_error(PLL_ERROR_PARAM_INVALID, "ancestral states: a result array is missing");
    if (b) b->failed = true;
    return PLL_FAILURE;
  }
  if (b->failed)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "ancestral states: the batch has failed already");
    return PLL_FAILURE;
  }
  Engine * e = engine_of(b->p);
  for (size_t k = 0; k < b->stages.size(); ++k)
  {
    if (!e->shards.empty()) push_model(b->p, e->shards[k]);
    if (!anc_stage_add(b->stages[k], b->flags, node_clv_index, other_clv_index, matrix_index, freqs_indices,
                       states, state_probs, probs))
    {
      b->failed = true;
      return PLL_FAILURE;
    }
  }
  return PLL_SUCCESS;
}

int pllhip_node_ancestral_finish(pllhip_anc_batch_t * b)
{
  if (!b) return PLL_SUCCESS;
  int ok = b->failed ? PLL_FAILURE : PLL_SUCCESS;
  double ms = 0.0;
  unsigned long long chunks = 0;
  for (AncStage & st : b->stages)
  {
    // (after a failure: whatever is in flight still has to leave the caller's arrays alone before they go away)
    if (b->failed) { if (st.p && st.d_buf) (void)hipStreamSynchronize(engine_of(st.p)->stream); }
    else if (!anc_stage_flush(st, b->flags)) ok = PLL_FAILURE;
    ms += st.kernel_ms;
    chunks = std::max(chunks, st.chunks);
    anc_stage_release(st);
  }
  g_anc_kernel_ms = ms;
  g_anc_chunks = chunks;
  delete b;
  return ok;
}

int pllhip_node_ancestral_batch(pll_partition_t * p, unsigned int count, const unsigned int * node_clv,
                                const unsigned int * other_clv, const unsigned int * matrix_indices,
                                const unsigned int * freqs_indices, unsigned int flags,
                                unsigned char * const * states, double * const * state_probs, double * const * probs)
{
  if (!count) return PLL_SUCCESS;
  if (!node_clv || !other_clv || !matrix_indices || !states || !state_probs || ((flags & PLLHIP_ANC_PROBS) && !probs))
  {
    set_error(PLL_ERROR_PARAM_INVALID, "ancestral states: an argument array is missing");
    return PLL_FAILURE;
  }
  pllhip_anc_batch_t * b = pllhip_node_ancestral_begin(p, flags, count);
  if (!b) return PLL_FAILURE;
  for (unsigned k = 0; k < count; ++k)
    if (!pllhip_node_ancestral_add(b, node_clv[k], other_clv[k], matrix_indices[k], freqs_indices, states[k],
                                   state_probs[k], (flags & PLLHIP_ANC_PROBS) ? probs[k] : nullptr))
      break;
  return pllhip_node_ancestral_finish(b);
}

void pllhip_node_ancestral_last_times(double * kernel_ms, unsigned long long * chunks)
{
  if (kernel_ms) *kernel_ms = g_anc_kernel_ms;
  if (chunks) *chunks = g_anc_chunks;
}

// ===========================================================================
// pllhip_* extension API
// ===========================================================================

int pllhip_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int pllhip_set_device(int device)
{
  int n = pllhip_device_count();
  if (device < 0 || device >= n)
  {
    set_error(PLL_ERROR_HIP_NODEVICE, "HIP device %d requested, %d visible", device, n);
    return PLL_FAILURE;
  }
  g_device = device;
  return PLL_SUCCESS;
}

int pllhip_get_device(void) { return current_device(); }

int pllhip_device_arch(int device, char * out, size_t out_len)
{
  hipDeviceProp_t prop;
  if (!hip_ok(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties")) return PLL_FAILURE;
  snprintf(out, out_len, "%s", prop.gcnArchName);
  return PLL_SUCCESS;
}

int pllhip_synchronize(pll_partition_t * p)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    for (pll_partition_t * c : e->shards) if (!pllhip_synchronize(c)) return PLL_FAILURE;
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  PLLHIP_TRY(hipStreamSynchronize(e->stream));
  return PLL_SUCCESS;
}

void * pllhip_stream(pll_partition_t * p) { return exec_engine(p)->stream; }

int pllhip_get_clv(pll_partition_t * p, unsigned int clv_index, double * out)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    // API layout is site-major: a shard's vector is a contiguous piece of the whole
    for (size_t k = 0; k < e->shards.size(); ++k)
      if (!pllhip_get_clv(e->shards[k], clv_index, out + (size_t)e->shard_first[k] * e->R * e->Sp)) return PLL_FAILURE;
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  if (!check_clv_index(e, clv_index, "requested")) return PLL_FAILURE;
  const size_t len = (size_t)e->N * e->R * e->Sp;
  if (!len) return PLL_SUCCESS;
  if (clv_index < e->tips && e->coded_tips)
  {
    double * tmp = nullptr;
    if (!upload_tipmap(p) || !dev_alloc(&tmp, len, "expanded tip")) return PLL_FAILURE;
    hipLaunchKernelGGL(k_expand_codes, dim3(reduce_grid(e)), dim3(256), 0, e->stream,
                       e->d_codes[clv_index], e->d_tipmap, e->N, e->R, e->S, e->Sp, tmp);
    PLLHIP_TRY(hipGetLastError());
    PLLHIP_TRY(hipMemcpyAsync(out, tmp, len * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    PLLHIP_TRY(hipStreamSynchronize(e->stream));
    (void)hipFree(tmp);
    return PLL_SUCCESS;
  }
  if (!need_clv(e, clv_index)) return PLL_FAILURE;
  return fetch_clv(e, e->d_clv[clv_index], out);
}

int pllhip_set_clv(pll_partition_t * p, unsigned int clv_index, const double * clv)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    for (size_t k = 0; k < e->shards.size(); ++k)
      if (!pllhip_set_clv(e->shards[k], clv_index, clv + (size_t)e->shard_first[k] * e->R * e->Sp)) return PLL_FAILURE;
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  if (!check_clv_index(e, clv_index, "target")) return PLL_FAILURE;
  if (clv_index < e->tips && e->coded_tips)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "CLV %u is a coded tip", clv_index);
    return PLL_FAILURE;
  }
  if (!transient_flush_all(e)) return PLL_FAILURE;            // (vectors that were not stored may read this one)
  if (e->shadow_codes && clv_index < e->tips) e->tip_has_codes[clv_index] = 0;
  if (!e->cherries.empty())
  {
    e->cherries[clv_index].valid = false;
    if (clv_index < e->tips) { e->tip_version[clv_index] = ++e->class_clock; e->plan.key.clear(); }
  }
  return store_clv(e, e->d_clv[clv_index], clv);
}

int pllhip_set_transient(pll_partition_t * p, int enable)
{
  Engine * e = engine_of(p);
  for (pll_partition_t * c : e->shards) (void)pllhip_set_transient(c, enable);
  e->transient_mode = enable != 0;
  return PLL_SUCCESS;
}

int pllhip_discard_transient(pll_partition_t * p)
{
  Engine * e = engine_of(p);
  for (pll_partition_t * c : e->shards) (void)pllhip_discard_transient(c);
  e->ledger.discard_mode_vectors();         // (a deferred store is not the caller's doing: it stays recomputable)
  return PLL_SUCCESS;
}

int pllhip_transient_stats(const pll_partition_t * p, pllhip_transient_stats_t * out)
{
  *out = exec_engine(p)->ledger.transient_stats();
  return PLL_SUCCESS;
}

int pllhip_deferred_stats(const pll_partition_t * p, pllhip_deferred_stats_t * out)
{
  *out = exec_engine(p)->ledger.deferred_stats();
  return PLL_SUCCESS;
}

int pllhip_schedule_stats(const pll_partition_t * p, pllhip_schedule_stats_t * out)
{
  const DevicePlan & dp = exec_engine(p)->plan;
  const bool resident = !dp.key.empty();
  out->chains = resident ? dp.nchains : 0;
  out->operations = resident ? dp.nops : 0;
  out->inner_reads = resident ? dp.inner_reads : 0;
  out->folded_cherries = resident ? dp.nfolds : 0;
  out->lookup_children = resident ? dp.nlookups : 0;
  return PLL_SUCCESS;
}

int pllhip_repeat_stats(const pll_partition_t * p, pllhip_repeat_stats_t * out)
{
  *out = exec_engine(p)->repeat_stats;
  return PLL_SUCCESS;
}

int pllhip_get_scaler(pll_partition_t * p, unsigned int idx, unsigned int * out)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    const size_t per = e->rate_scalers ? e->R : 1;
    for (size_t k = 0; k < e->shards.size(); ++k)
      if (!pllhip_get_scaler(e->shards[k], idx, out + (size_t)e->shard_first[k] * per)) return PLL_FAILURE;
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  if (idx >= e->nscalers) { set_error(PLL_ERROR_PARAM_INVALID, "scaler index out of range"); return PLL_FAILURE; }
  if (!e->N) return PLL_SUCCESS;
  if (!need_scaler(e, (int)idx)) return PLL_FAILURE;
  PLLHIP_TRY(hipMemcpyAsync(out, e->d_scalers + (size_t)idx * e->sc_len,
                            sizeof(unsigned) * e->N * (e->rate_scalers ? e->R : 1),
                            hipMemcpyDeviceToHost, e->stream));
  PLLHIP_TRY(hipStreamSynchronize(e->stream));
  return PLL_SUCCESS;
}

int pllhip_set_scaler(pll_partition_t * p, unsigned int idx, const unsigned int * in)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    const size_t per = e->rate_scalers ? e->R : 1;
    for (size_t k = 0; k < e->shards.size(); ++k)
      if (!pllhip_set_scaler(e->shards[k], idx, in + (size_t)e->shard_first[k] * per)) return PLL_FAILURE;
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  if (idx >= e->nscalers) { set_error(PLL_ERROR_PARAM_INVALID, "scaler index out of range"); return PLL_FAILURE; }
  if (!e->N) return PLL_SUCCESS;
  if (!transient_flush_all(e)) return PLL_FAILURE;
  if (idx < e->scaler_lazy.size()) e->scaler_lazy[idx] = -1;         // the caller's counts replace whatever stood for the buffer
  PLLHIP_TRY(hipMemcpyAsync(e->d_scalers + (size_t)idx * e->sc_len, in,
                            sizeof(unsigned) * e->N * (e->rate_scalers ? e->R : 1),
                            hipMemcpyHostToDevice, e->stream));
  PLLHIP_TRY(hipStreamSynchronize(e->stream));
  return PLL_SUCCESS;
}

int pllhip_get_sumtable(pll_partition_t * p, const double * key, double * out)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    for (size_t k = 0; k < e->shards.size(); ++k)
      if (!pllhip_get_sumtable(e->shards[k], key, out + (size_t)e->shard_first[k] * e->R * e->Sp)) return PLL_FAILURE;
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  double * d_sum = sumtable_device(e, key, false);
  if (!d_sum) { set_error(PLL_ERROR_PARAM_INVALID, "unknown sumtable key"); return PLL_FAILURE; }
  return fetch_clv(e, d_sum, out);
}

int pllhip_sync_to_host(pll_partition_t * p, unsigned int what)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty() && (what & PLLHIP_SYNC_PMATRIX) && e->nmat)
  {
    // every shard holds the same matrices: the first one's mirror is the partition's
    pll_partition_t * c = e->shards[0];
    if (!pllhip_sync_to_host(c, PLLHIP_SYNC_PMATRIX)) return PLL_FAILURE;
    memcpy(p->pmatrix[0], c->pmatrix[0], sizeof(double) * (size_t)e->nmat * e->R * e->S * e->Sp);
    what &= ~(unsigned)PLLHIP_SYNC_PMATRIX;
  }
  if (e->shards.empty()) PLLHIP_TRY(hipSetDevice(e->device));
  if ((what & PLLHIP_SYNC_PMATRIX) && e->pmat_host_dirty && e->nmat)
  {
    if (!flush_pmatrices(p)) return PLL_FAILURE;
    PLLHIP_TRY(hipMemcpyAsync(p->pmatrix[0], e->d_pmat,
                              sizeof(double) * (size_t)e->nmat * e->R * e->S * e->Sp,
                              hipMemcpyDeviceToHost, e->stream));
    PLLHIP_TRY(hipStreamSynchronize(e->stream));
    e->pmat_host_dirty = false;
  }
  if (what & PLLHIP_SYNC_CLV)
  {
    const size_t len = (size_t)e->N * e->R * e->Sp;
    for (unsigned i = 0; i < e->nodes; ++i)
    {
      if (i < e->tips && e->coded_tips) continue;   // libpll keeps no CLV for coded tips either
      if (!p->clv[i]) p->clv[i] = static_cast<double *>(pll_aligned_alloc(sizeof(double) * (len ? len : 1), p->alignment));
      if (!p->clv[i]) { set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate host CLV mirror"); return PLL_FAILURE; }
      if (!pllhip_get_clv(p, i, p->clv[i])) return PLL_FAILURE;
    }
  }
  if (what & PLLHIP_SYNC_SCALERS)
    for (unsigned i = 0; i < e->nscalers; ++i)
    {
      if (!p->scale_buffer[i])
        p->scale_buffer[i] = static_cast<unsigned *>(calloc((e->N ? e->N : 1) * (e->rate_scalers ? (size_t)e->R : 1),
                                                            sizeof(unsigned)));
      if (!p->scale_buffer[i]) { set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate host scaler mirror"); return PLL_FAILURE; }
      if (!pllhip_get_scaler(p, i, p->scale_buffer[i])) return PLL_FAILURE;
    }
  // a dump of this partition tells the loader to create one with host mirrors again
  if (what & (PLLHIP_SYNC_CLV | PLLHIP_SYNC_SCALERS)) p->attributes |= PLLHIP_ATTRIB_HOST_MIRRORS;
  return PLL_SUCCESS;
}

int pllhip_sync_to_device(pll_partition_t * p, unsigned int what)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty() && (what & PLLHIP_SYNC_PMATRIX) && e->nmat)
  {
    for (pll_partition_t * c : e->shards)
    {
      memcpy(c->pmatrix[0], p->pmatrix[0], sizeof(double) * (size_t)e->nmat * e->R * e->S * e->Sp);
      if (!pllhip_sync_to_device(c, PLLHIP_SYNC_PMATRIX)) return PLL_FAILURE;
    }
    what &= ~(unsigned)PLLHIP_SYNC_PMATRIX;
  }
  if (!e->shards.empty())
    for (pll_partition_t * c : e->shards) push_model(p, c);     // a loader filled the parent's model arrays
  if (e->shards.empty()) PLLHIP_TRY(hipSetDevice(e->device));
  if (e->shards.empty() && !transient_flush_all(e)) return PLL_FAILURE;
  e->eigen_touched = true;                                  // a loader may have filled the model arrays
  e->pmatrix_burst = false;
  if (what & PLLHIP_SYNC_TIPS)
  {
    if (e->coded_tips)
    {
      e->tipmap_codes_uploaded = ~0u;                       // the map itself may be new
      for (unsigned t = 0; t < e->tips; ++t)
        if (p->tipchars && p->tipchars[t] && !upload_tip_codes(p, t)) return PLL_FAILURE;
      invalidate_luts(p);
    }
    p->pattern_weight_sum = 0;
    for (unsigned i = 0; i < p->sites; ++i) p->pattern_weight_sum += p->pattern_weights[i];
    if (!upload_weights(p)) return PLL_FAILURE;
    e->invariant_uploaded = false;
  }
  if ((what & PLLHIP_SYNC_PMATRIX) && e->nmat)
  {
    // the host mirror is the truth now: queued requests are obsolete
    for (unsigned m : e->pend_midx) e->pend_pos[m] = -1;
    e->pend_midx.clear();
    e->pend_t.clear();
    PLLHIP_TRY(hipMemcpyAsync(e->d_pmat, p->pmatrix[0],
                              sizeof(double) * (size_t)e->nmat * e->R * e->S * e->Sp,
                              hipMemcpyHostToDevice, e->stream));
    PLLHIP_TRY(hipStreamSynchronize(e->stream));
    e->pmat_host_dirty = false;
    invalidate_luts(p);
    if (e->d_pfrag)
    {
      hipLaunchKernelGGL(k_s20_pfrag, dim3(e->nmat), dim3(256), 0, e->stream, e->d_pmat, e->d_pfrag, e->R);
      PLLHIP_TRY(hipGetLastError());
    }
  }
  if (what & PLLHIP_SYNC_CLV)
    for (unsigned i = 0; i < e->nodes; ++i)
    {
      if ((i < e->tips && e->coded_tips) || !p->clv[i]) continue;
      if (!pllhip_set_clv(p, i, p->clv[i])) return PLL_FAILURE;
    }
  if (what & PLLHIP_SYNC_SCALERS)
    for (unsigned i = 0; i < e->nscalers; ++i)
      if (p->scale_buffer[i] && !pllhip_set_scaler(p, i, p->scale_buffer[i])) return PLL_FAILURE;
  return PLL_SUCCESS;
}

int pllhip_get_counters(const pll_partition_t * p, pllhip_counters_t * out)
{
  // a sharded partition reports its first shard: every shard does the same calls on its share of the sites
  *out = exec_engine(p)->counters;
  return PLL_SUCCESS;
}

void pllhip_reset_counters(pll_partition_t * p)
{
  engine_of(p)->counters = pllhip_counters_t{};
  for (pll_partition_t * c : engine_of(p)->shards) engine_of(c)->counters = pllhip_counters_t{};
}

int pllhip_profile_partials(pll_partition_t * p, int enable)
{
  Engine * e = engine_of(p);
  for (pll_partition_t * c : e->shards) (void)pllhip_profile_partials(c, enable);
  e->profiling = enable != 0;
  e->prof_used = 0;
  e->prof_bytes = 0.0;
  e->prof_min_bytes = 0.0;
  e->prof_flops = 0.0;
  e->prof_ops = 0;
  return PLL_SUCCESS;
}

int pllhip_profile_read(pll_partition_t * p, pllhip_profile_t * out)
{
  Engine * e = engine_of(p);
  if (!e->shards.empty())
  {
    // bytes and flops add up over the shards; the devices run side by side, so the time is the slowest shard's
    memset(out, 0, sizeof(*out));
    for (pll_partition_t * c : e->shards)
    {
      pllhip_profile_t one;
      if (!pllhip_profile_read(c, &one)) return PLL_FAILURE;
      out->launches = one.launches;
      out->ops = one.ops;
      out->kernel_ms = std::max(out->kernel_ms, one.kernel_ms);
      out->algorithmic_bytes += one.algorithmic_bytes;
      out->algorithmic_flops += one.algorithmic_flops;
      out->minimum_bytes += one.minimum_bytes;
    }
    return PLL_SUCCESS;
  }
  PLLHIP_TRY(hipSetDevice(e->device));
  PLLHIP_TRY(hipStreamSynchronize(e->stream));
  double ms = 0.0;
  for (size_t k = 0; k < e->prof_used; ++k)
  {
    float t = 0.0f;
    PLLHIP_TRY(hipEventElapsedTime(&t, e->prof_events[k].first, e->prof_events[k].second));
    ms += t;
  }
  out->launches = e->prof_used;
  out->ops = e->prof_ops;
  out->kernel_ms = ms;
  out->algorithmic_bytes = e->prof_bytes;
  out->algorithmic_flops = e->prof_flops;
  out->minimum_bytes = e->prof_min_bytes;
  e->prof_used = 0;
  e->prof_bytes = 0.0;
  e->prof_min_bytes = 0.0;
  e->prof_flops = 0.0;
  e->prof_ops = 0;
  return PLL_SUCCESS;
}

const char * pllhip_partials_kernel_name(const pll_partition_t * p)
{
  return edge_family(exec_engine(p))->name;
}

} // extern "C"
