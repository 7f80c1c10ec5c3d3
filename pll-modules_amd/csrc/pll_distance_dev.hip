// pll_distance_dev.hip -- pairwise distances from tips that live on the device, and neighbour joining
// (kernels_distance.hpp; contract: INTEGRATION.md, "Pairwise distances and neighbour joining"; design: DESIGN.md
// section 23).
//
// A call stages the sites as columns of weight 1 .. 127 (a heavier pattern becomes several columns), turns every
// character into a one-byte code, and walks the taxa in bands whose rows of the count table fit the budget: the
// integer product fills the band's rows, the distance kernel reads them.  The partition form runs on the partition's
// stream, the alignment form and neighbour joining on a stream of their own on the device pllhip_get_device() names.
#include "device_job.hpp"
#include "kernels_distance.hpp"
#include "msa_upload.hpp"
#include "nj_tree.h"
#include "pllhip.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pllhip;

struct pllhip_distmat
{
  unsigned T = 0, S = 0;
  int device = 0;
  std::vector<double> D;                 // [T][T]
  std::vector<unsigned> compared;        // [T][T]
  unsigned long long no_overlap = 0;
  int * d_counts = nullptr;              // [T * S][T * S] under PLLHIP_DIST_KEEP_COUNTS
  bool joined = false;
  std::vector<unsigned> slots;           // the join list, 2 (T - 3) + 3
  std::vector<double> lengths;
};

namespace {

using u64 = unsigned long long;

constexpr size_t DIST_STAGE_BYTES = (size_t)16 << 20;
constexpr u64 DIST_DEFAULT_BUDGET = 1ULL << 30;
constexpr unsigned DIST_TARGET_WAVES = 4096;                  // waves the product aims for when it splits the columns

thread_local double g_last_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // upload, codes, counts, estimate, nj

struct Settings
{
  int method = PLLHIP_DIST_P;
  unsigned flags = 0;
  double dmin = 1e-6, dmax = 10.0;
  u64 budget = DIST_DEFAULT_BUDGET;
  unsigned chunk = 0;
};

bool read_params(const pllhip_dist_params_t * params, bool partition_form, Settings & s, const char * who)
{
  if (!params)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL parameters", who);
    return false;
  }
  s.method = params->method;
  s.flags = params->flags;
  if (s.method != PLLHIP_DIST_P && s.method != PLLHIP_DIST_JC && !(partition_form && s.method == PLLHIP_DIST_ML))
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: method %d is not offered here", who, s.method);
    return false;
  }
  if (params->min_dist != 0.0) s.dmin = params->min_dist;
  if (params->max_dist != 0.0) s.dmax = params->max_dist;
  if (!(s.dmin > 0.0) || !(s.dmax > s.dmin) || !std::isfinite(s.dmax))
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: 0 < min_dist < max_dist does not hold (%g, %g)", who, s.dmin, s.dmax);
    return false;
  }
  if (params->budget_bytes) s.budget = params->budget_bytes;
  else if (const char * mb = getenv("PLLHIP_DIST_BUDGET_MB"))
  {
    const u64 v = strtoull(mb, nullptr, 10);
    if (v) s.budget = v << 20;
  }
  s.chunk = params->chunk_columns;
  return true;
}

// where the characters come from, and what the ML distance needs of the model (host pointers; R = 0: no model)
struct Source
{
  TipView view = {};
  bool coded = false;
  const u64 * d_tipmap = nullptr;
  unsigned T = 0, N = 0, S = 0;
  const unsigned * weights = nullptr;          // host, [N]; NULL: all 1
  const pll_partition_t * model = nullptr;
};

// the sites as columns of weight 1 .. 127
bool stage_columns(const Source & src, std::vector<unsigned> & col_site, std::vector<uint8_t> & col_w, const char * who)
{
  u64 sum = 0;
  for (unsigned n = 0; n < src.N; ++n) sum += src.weights ? src.weights[n] : 1u;
  if (sum >= (1ULL << 31))
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: the weights add up to %llu; the counts are 32-bit (less than 2^31)", who, sum);
    return false;
  }
  for (unsigned n = 0; n < src.N; ++n)
    for (unsigned w = src.weights ? src.weights[n] : 1u; w; )
    {
      const unsigned part = std::min(w, DST_MAX_W);
      col_site.push_back(n);
      col_w.push_back((uint8_t)part);
      w -= part;
    }
  return true;
}

// codes, counts and distances of `src` on the job's stream.  *bad = tip * sites + site of an unmapped character
// (DST_NO_BAD: none; the caller words the error).
pllhip_distmat * compute(DeviceJob & j, const Source & src, const Settings & st, int device, double upload_ms, u64 * bad,
                         const char * who)
{
  const unsigned T = src.T, S = src.S;
  std::vector<unsigned> col_site;
  std::vector<uint8_t> col_w;
  if (!stage_columns(src, col_site, col_w, who)) return nullptr;
  const unsigned C = (unsigned)col_site.size();
  const u64 Cpad = std::max<u64>(DST_KSTEP, ((u64)C + DST_KSTEP - 1) / DST_KSTEP * DST_KSTEP);
  const u64 M = (u64)T * S;
  const u64 col_tiles = (M + DST_TILE - 1) / DST_TILE;
  if (col_tiles > 65535u || T > 65535u || col_site.size() > 0xFFFFFFFFull)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: %u taxa of %u states are more than the count table holds", who, T, S);
    return nullptr;
  }
  // taxa per band
  const u64 taxon_bytes = (u64)S * M * sizeof(int);
  unsigned band = (unsigned)std::min<u64>(T, std::max<u64>(1, st.budget / taxon_bytes));
  const bool keep = (st.flags & PLLHIP_DIST_KEEP_COUNTS) != 0;
  if (keep && band < T)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: PLLHIP_DIST_KEEP_COUNTS needs %llu bytes for the counts; the budget is %llu",
              who, taxon_bytes * T, st.budget);
    return nullptr;
  }

  hipEvent_t ev[4] = {j.event(), j.event(), j.event(), j.event()};      // start, staged, coded; band marks
  hipEvent_t evb = j.event(), evc = j.event();
  for (hipEvent_t e : ev) if (!e) return nullptr;
  if (!evb || !evc) return nullptr;

  unsigned * d_site = j.alloc<unsigned>(C, "the site list");
  uint8_t * d_wq = j.alloc<uint8_t>(Cpad, "column weights");
  uint8_t * d_codes = j.alloc<uint8_t>((size_t)T * Cpad, "codes");
  u64 * d_status = j.alloc<u64>(3, "status words");
  int * d_counts = j.alloc<int>((size_t)band * S * M, "the count table");
  double * d_D = j.alloc<double>((size_t)T * T, "the distance matrix");
  unsigned * d_cmp = j.alloc<unsigned>((size_t)T * T, "compared sites");
  if (!d_site || !d_wq || !d_codes || !d_status || !d_counts || !d_D || !d_cmp) return nullptr;

  // the model of the ML distance
  DstModel md = {};
  if (st.method == PLLHIP_DIST_ML)
  {
    const pll_partition_t * p = src.model;
    const size_t SSp = (size_t)S * p->states_padded;
    double * d_model = j.alloc<double>(2 * SSp + p->states_padded + 2 * p->rate_cats, "the model");
    if (!d_model) return nullptr;
    md.V = d_model; md.Vi = d_model + SSp; md.evals = d_model + 2 * SSp;
    md.rates = md.evals + p->states_padded; md.rate_w = md.rates + p->rate_cats;
    md.R = p->rate_cats; md.Sp = p->states_padded; md.pinv = p->prop_invar[0];
    if (!j.upload(d_model, p->inv_eigenvecs[0], SSp, "upload model") ||
        !j.upload(d_model + SSp, p->eigenvecs[0], SSp, "upload model") ||
        !j.upload(d_model + 2 * SSp, p->eigenvals[0], (size_t)p->states_padded, "upload model") ||
        !j.upload(d_model + 2 * SSp + p->states_padded, p->rates, (size_t)p->rate_cats, "upload model") ||
        !j.upload(d_model + 2 * SSp + p->states_padded + p->rate_cats, p->rate_weights, (size_t)p->rate_cats,
                  "upload model"))
      return nullptr;
  }

  const u64 status0[3] = {DST_NO_BAD, 0, 0};
  if (!hip_ok(hipEventRecord(ev[0], j.stream), "hipEventRecord") ||
      (C && !j.upload(d_site, col_site.data(), (size_t)C, "upload site list")) ||
      !hip_ok(hipMemsetAsync(d_wq, 0, Cpad, j.stream), "memset weights") ||
      (C && !j.upload(d_wq, col_w.data(), (size_t)C, "upload column weights")) ||
      !j.upload(d_status, status0, 3, "upload status") ||
      !hip_ok(hipEventRecord(ev[1], j.stream), "hipEventRecord"))
    return nullptr;

  {
    const dim3 grid((unsigned)((Cpad + DST_WG - 1) / DST_WG), std::min(T, 4096u));
    if (src.coded)
      hipLaunchKernelGGL((k_dst_codes<true>), grid, dim3(DST_WG), 0, j.stream, src.view, src.d_tipmap, d_site, T, src.N, S,
                         C, Cpad, d_codes, d_status);
    else
      hipLaunchKernelGGL((k_dst_codes<false>), grid, dim3(DST_WG), 0, j.stream, src.view, src.d_tipmap, d_site, T, src.N,
                         S, C, Cpad, d_codes, d_status);
  }
  u64 status[3] = {0, 0, 0};
  if (!hip_ok(hipGetLastError(), "code kernel") || !hip_ok(hipEventRecord(ev[2], j.stream), "hipEventRecord") ||
      !hip_ok(hipMemcpyAsync(status, d_status, sizeof(status), hipMemcpyDeviceToHost, j.stream), "download status") ||
      !hip_ok(hipStreamSynchronize(j.stream), "code kernel"))
    return nullptr;
  *bad = status[DST_BAD];
  if (*bad != DST_NO_BAD) return nullptr;
  if (status[DST_NONBIN])
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: a tip vector holds an entry other than 0 and 1; distances need states", who);
    return nullptr;
  }

  // columns per wave: enough waves to fill the device where the table is small
  const u64 tiles = col_tiles * (col_tiles + 1) / 2;
  u64 chunk = st.chunk ? st.chunk : (Cpad * tiles + DIST_TARGET_WAVES - 1) / DIST_TARGET_WAVES;
  chunk = std::max<u64>(DST_KSTEP, (chunk + DST_KSTEP - 1) / DST_KSTEP * DST_KSTEP);
  chunk = std::max<u64>(chunk, ((Cpad + 65534) / 65535 + DST_KSTEP - 1) / DST_KSTEP * DST_KSTEP);
  const unsigned splits = (unsigned)((Cpad + chunk - 1) / chunk);

  double counts_ms = 0.0, estimate_ms = 0.0;
  if (!hip_ok(hipMemsetAsync(d_status + 2, 0, sizeof(u64), j.stream), "memset")) return nullptr;
  for (unsigned t0 = 0; t0 < T; t0 += band)
  {
    const unsigned nt = std::min(band, T - t0), rows = nt * S;
    if (!hip_ok(hipMemsetAsync(d_counts, 0, (size_t)rows * M * sizeof(int), j.stream), "memset counts") ||
        !hip_ok(hipEventRecord(ev[3], j.stream), "hipEventRecord"))
      return nullptr;
    hipLaunchKernelGGL(k_dst_counts, dim3((unsigned)col_tiles, (rows + DST_TILE - 1) / DST_TILE, splits), dim3(64), 0,
                       j.stream, d_codes, d_wq, Cpad, S, t0 * S, rows, (unsigned)M, chunk, d_counts);
    if (!hip_ok(hipGetLastError(), "count kernel") || !hip_ok(hipEventRecord(evb, j.stream), "hipEventRecord")) return nullptr;
    hipLaunchKernelGGL(k_dst_estimate, dim3(T, nt), dim3(64), 0, j.stream, d_counts, t0, (unsigned)M, S, T, md, st.method,
                       st.dmin, st.dmax, d_D, d_cmp, d_status + 2);
    float a = 0.f, b = 0.f;
    if (!hip_ok(hipGetLastError(), "distance kernel") || !hip_ok(hipEventRecord(evc, j.stream), "hipEventRecord") ||
        !hip_ok(hipStreamSynchronize(j.stream), "distance kernels") ||
        !hip_ok(hipEventElapsedTime(&a, ev[3], evb), "hipEventElapsedTime") ||
        !hip_ok(hipEventElapsedTime(&b, evb, evc), "hipEventElapsedTime"))
      return nullptr;
    counts_ms += a;
    estimate_ms += b;
  }

  pllhip_distmat * dm = new pllhip_distmat;
  dm->T = T; dm->S = S; dm->device = device;
  dm->D.resize((size_t)T * T);
  dm->compared.resize((size_t)T * T);
  float up = 0.f, codes = 0.f;
  if (!hip_ok(hipMemcpyAsync(dm->D.data(), d_D, (size_t)T * T * sizeof(double), hipMemcpyDeviceToHost, j.stream), "download") ||
      !hip_ok(hipMemcpyAsync(dm->compared.data(), d_cmp, (size_t)T * T * sizeof(unsigned), hipMemcpyDeviceToHost, j.stream),
              "download") ||
      !hip_ok(hipMemcpyAsync(&dm->no_overlap, d_status + 2, sizeof(u64), hipMemcpyDeviceToHost, j.stream), "download") ||
      !hip_ok(hipStreamSynchronize(j.stream), "download") ||
      !hip_ok(hipEventElapsedTime(&up, ev[0], ev[1]), "hipEventElapsedTime") ||
      !hip_ok(hipEventElapsedTime(&codes, ev[1], ev[2]), "hipEventElapsedTime"))
  {
    delete dm;
    return nullptr;
  }
  if (keep) { dm->d_counts = d_counts; j.keep(d_counts); }
  g_last_ms[0] = upload_ms + up;
  g_last_ms[1] = codes;
  g_last_ms[2] = counts_ms;
  g_last_ms[3] = estimate_ms;
  return dm;
}

bool check_states(unsigned states, const char * who)
{
  if (states >= 2 && states <= DST_MAX_STATES) return true;
  set_error(PLL_ERROR_PARAM_INVALID, "%s: %u states (2 to %u are supported)", who, states, DST_MAX_STATES);
  return false;
}

// neighbour joining of dm->D: the join list into dm->slots / dm->lengths
bool run_nj(pllhip_distmat * dm)
{
  const unsigned T = dm->T, rounds = T - 3, entries = 2 * rounds + 3;
  const auto t_begin = std::chrono::steady_clock::now();
  DeviceJob j;
  if (!j.enter(dm->device)) return false;
  double * d_D = j.alloc<double>((size_t)T * T, "the distance matrix");
  double * d_r = j.alloc<double>(T, "row sums");
  unsigned * d_alive = j.alloc<unsigned>(T, "active slots");
  NjKey * d_min = j.alloc<NjKey>(NJ_MAX_GRID, "minima");
  unsigned * d_slots = j.alloc<unsigned>(entries, "joins");
  double * d_len = j.alloc<double>(entries, "joins");
  if (!d_D || !d_r || !d_alive || !d_min || !d_slots || !d_len) return false;
  std::vector<unsigned> alive(T);
  for (unsigned i = 0; i < T; ++i) alive[i] = i;
  if (!j.upload(d_D, dm->D.data(), (size_t)T * T, "upload matrix") || !j.upload(d_alive, alive.data(), (size_t)T, "upload slots") ||
      !hip_ok(hipMemsetAsync(d_slots, 0xff, entries * sizeof(unsigned), j.stream), "memset joins"))
    return false;
  hipLaunchKernelGGL(k_nj_rowsum, dim3((T + DST_WG - 1) / DST_WG), dim3(DST_WG), 0, j.stream, d_D, T, d_r);
  for (unsigned q = 0; q < rounds; ++q)
  {
    const unsigned n = T - q, blocks = std::min(n - 1, NJ_MAX_GRID);
    hipLaunchKernelGGL(k_nj_min, dim3(blocks), dim3(DST_WG), 0, j.stream, d_D, d_r, d_alive, n, T, d_min);
    hipLaunchKernelGGL(k_nj_join, dim3(1), dim3(DST_WG), 0, j.stream, d_D, d_r, d_alive, n, T, d_min, blocks, q, d_slots,
                       d_len);
  }
  hipLaunchKernelGGL(k_nj_last, dim3(1), dim3(64), 0, j.stream, d_D, d_alive, T, rounds, d_slots, d_len);
  dm->slots.assign(entries, 0);
  dm->lengths.assign(entries, 0.0);
  if (!hip_ok(hipGetLastError(), "neighbour-joining kernels") ||
      !hip_ok(hipMemcpyAsync(dm->slots.data(), d_slots, entries * sizeof(unsigned), hipMemcpyDeviceToHost, j.stream), "download") ||
      !hip_ok(hipMemcpyAsync(dm->lengths.data(), d_len, entries * sizeof(double), hipMemcpyDeviceToHost, j.stream), "download") ||
      !hip_ok(hipStreamSynchronize(j.stream), "neighbour-joining kernels"))
    return false;
  for (unsigned s : dm->slots)
    if (s >= T)
    {
      set_error(PLL_ERROR_PARAM_INVALID, "pllhip_distmat_nj: the matrix gave no join (a value that is not finite)");
      return false;
    }
  dm->joined = true;
  g_last_ms[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return true;
}

} // namespace

extern "C" {

PLL_EXPORT pllhip_distmat_t * pllhip_distances_partition(pll_partition_t * partition, const pllhip_dist_params_t * params)
{
  const char * who = "pllhip_distances_partition";
  if (!partition || !partition->engine)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL partition", who);
    return nullptr;
  }
  Settings st;
  if (!check_states(partition->states, who) || !read_params(params, true, st, who)) return nullptr;
  Engine * e = engine_of(partition);
  if (!e->shards.empty())
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: sharded partitions are not supported", who);
    return nullptr;
  }
  if (partition->tips < 2)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: %u tips", who, partition->tips);
    return nullptr;
  }
  if (st.method == PLLHIP_DIST_ML)
  {
    if (partition->rate_matrices > 1)
    {
      set_error(PLL_ERROR_PARAM_INVALID, "%s: PLLHIP_DIST_ML takes one rate matrix; the partition has %u", who,
                partition->rate_matrices);
      return nullptr;
    }
    if (!partition->eigen_decomp_valid[0] && !pll_update_eigen(partition, 0)) return nullptr;
  }
  DeviceJob j;
  DevBuf<const double *> d_clv;
  DevBuf<const uint8_t *> d_rows;
  if (!j.enter(e->device, e->stream) || !upload_tipmap(partition) || !tip_pointer_tables(e, d_clv, d_rows))
    return nullptr;
  Source src;
  src.view.code_rows = d_rows.p;
  src.view.clv_rows = d_clv.p;
  src.view.R = e->R;
  src.view.Sp = e->Sp;
  src.view.brows = e->rows;
  src.coded = e->coded_tips;
  src.d_tipmap = e->coded_tips ? e->d_tipmap : nullptr;
  src.T = e->tips;
  src.N = e->Nreal;
  src.S = e->S;
  src.weights = partition->pattern_weights;
  src.model = partition;
  u64 bad = DST_NO_BAD;
  pllhip_distmat * dm = compute(j, src, st, e->device, 0.0, &bad, who);
  if (!dm && bad != DST_NO_BAD)
    set_error(PLL_ERROR_MSA_MAP_INVALID, "%s: tip %llu holds a code without a state at site %llu", who, bad / src.N + 1,
              bad % src.N + 1);
  return dm;
}

PLL_EXPORT pllhip_distmat_t * pllhip_distances_msa(const pll_msa_t * msa, unsigned int states, const pll_state_t * tipmap,
                                                   const unsigned int * weights, const pllhip_dist_params_t * params)
{
  const char * who = "pllhip_distances_msa";
  if (!msa || !tipmap)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: %s is NULL", who, msa ? "Character-to-state mapping" : "MSA structure");
    return nullptr;
  }
  Settings st;
  if (!check_states(states, who) || !read_params(params, false, st, who)) return nullptr;
  if (msa->count < 2 || msa->length < 1 || !msa->sequence)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: fewer than two sequences, or no site", who);
    return nullptr;
  }
  for (int t = 0; t < msa->count; ++t)
    if (!msa->sequence[t])
    {
      set_error(PLL_ERROR_PARAM_INVALID, "%s: sequence %d is NULL", who, t);
      return nullptr;
    }
  int device = 0;
  if (!caller_device(who, &device)) return nullptr;
  const unsigned T = (unsigned)msa->count, L = (unsigned)msa->length;
  const size_t Lp = ((size_t)L + 255u) & ~(size_t)255u;
  const size_t half = std::min(DIST_STAGE_BYTES, (size_t)T * Lp);
  DeviceJob j;
  MsaStager stager;
  if (!j.enter(device)) return nullptr;
  hipEvent_t e0 = j.event(), e1 = j.event();
  uint8_t * d_in = j.alloc<uint8_t>((size_t)T * Lp, "the alignment");
  u64 * d_map = j.alloc<u64>(256, "the character map");
  if (!e0 || !e1 || !d_in || !d_map || !stager.open(half)) return nullptr;
  float up = 0.f;
  if (!hip_ok(hipEventRecord(e0, j.stream), "hipEventRecord") ||
      !stager.rows(j.stream, d_in, msa->sequence, T, L, Lp, half) ||
      !j.upload(d_map, (const u64 *)tipmap, 256, "upload map") || !hip_ok(hipEventRecord(e1, j.stream), "hipEventRecord") ||
      !hip_ok(hipStreamSynchronize(j.stream), "upload alignment") || !j.elapsed(e0, e1, &up))
    return nullptr;
  Source src;
  src.view.code_base = d_in;
  src.view.code_stride = Lp;
  src.coded = true;
  src.d_tipmap = d_map;
  src.T = T;
  src.N = L;
  src.S = states;
  src.weights = weights;
  u64 bad = DST_NO_BAD;
  pllhip_distmat * dm = compute(j, src, st, device, up, &bad, who);
  if (!dm && bad != DST_NO_BAD)
  {
    const u64 t = bad / L, s = bad % L;
    const char c = msa->sequence[t][s];
    if (c == (char)-1) set_error(PLL_ERROR_MSA_MAP_INVALID, "Unknown state in sequence %llu", t + 1);
    else set_error(PLL_ERROR_MSA_MAP_INVALID, "Unknown state %c at sequence %llu position %llu", c, t + 1, s + 1);
  }
  return dm;
}

PLL_EXPORT pllhip_distmat_t * pllhip_distmat_from_host(unsigned int T, const double * matrix)
{
  const char * who = "pllhip_distmat_from_host";
  if (T < 3 || T > 46340u || !matrix)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: %u taxa (3 to 46340), or no matrix", who, T);
    return nullptr;
  }
  for (size_t k = 0; k < (size_t)T * T; ++k)
    if (!std::isfinite(matrix[k]))
    {
      set_error(PLL_ERROR_PARAM_INVALID, "%s: entry (%zu, %zu) is not finite", who, k / T, k % T);
      return nullptr;
    }
  int device = 0;
  if (!caller_device(who, &device)) return nullptr;
  pllhip_distmat * dm = new pllhip_distmat;
  dm->T = T;
  dm->device = device;
  dm->D.assign(matrix, matrix + (size_t)T * T);
  dm->compared.assign((size_t)T * T, 0u);
  return dm;
}

PLL_EXPORT void pllhip_distmat_destroy(pllhip_distmat_t * dm)
{
  if (!dm) return;
  if (dm->d_counts)
  {
    DeviceScope scope;
    (void)scope.enter(dm->device);
    (void)hipFree(dm->d_counts);
  }
  delete dm;
}

PLL_EXPORT unsigned int pllhip_distmat_size(const pllhip_distmat_t * dm) { return dm ? dm->T : 0; }

PLL_EXPORT int pllhip_distmat_get(const pllhip_distmat_t * dm, double * out)
{
  if (!dm || !out)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_distmat_get: NULL argument");
    return PLL_FAILURE;
  }
  memcpy(out, dm->D.data(), dm->D.size() * sizeof(double));
  return PLL_SUCCESS;
}

PLL_EXPORT int pllhip_distmat_compared(const pllhip_distmat_t * dm, unsigned int * out)
{
  if (!dm || !out)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_distmat_compared: NULL argument");
    return PLL_FAILURE;
  }
  memcpy(out, dm->compared.data(), dm->compared.size() * sizeof(unsigned));
  return PLL_SUCCESS;
}

PLL_EXPORT int pllhip_distmat_counts(const pllhip_distmat_t * dm, unsigned int i, unsigned int j, int * out)
{
  if (!dm || !out || i >= dm->T || j >= dm->T)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_distmat_counts: NULL argument or a taxon out of range");
    return PLL_FAILURE;
  }
  if (!dm->d_counts)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_distmat_counts: the matrix was made without PLLHIP_DIST_KEEP_COUNTS");
    return PLL_FAILURE;
  }
  // the table holds the blocks on and above the diagonal: N_ij = N_ji^T
  const unsigned S = dm->S, lo = std::min(i, j), hi = std::max(i, j);
  const size_t M = (size_t)dm->T * S;
  std::vector<int> blk((size_t)S * S);
  DeviceScope scope;
  if (!scope.enter(dm->device)) return PLL_FAILURE;
  PLLHIP_TRY(hipMemcpy2D(blk.data(), S * sizeof(int), dm->d_counts + (size_t)lo * S * M + (size_t)hi * S, M * sizeof(int),
                         S * sizeof(int), S, hipMemcpyDeviceToHost));
  for (unsigned a = 0; a < S; ++a)
    for (unsigned b = 0; b < S; ++b)
    {
      int v = i <= j ? blk[(size_t)a * S + b] : blk[(size_t)b * S + a];
      if (i == j && a != b) v = 0;                       // (one code per character; below the diagonal nothing is made)
      out[(size_t)a * S + b] = v;
    }
  return PLL_SUCCESS;
}

PLL_EXPORT unsigned long long pllhip_distmat_no_overlap(const pllhip_distmat_t * dm) { return dm ? dm->no_overlap : 0; }

PLL_EXPORT int pllhip_distmat_nj_joins(pllhip_distmat_t * dm, unsigned int * slots, double * lengths)
{
  if (!dm || !slots || !lengths || dm->T < 3)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_distmat_nj_joins: NULL argument, or fewer than 3 taxa");
    return PLL_FAILURE;
  }
  if (!dm->joined && !run_nj(dm)) return PLL_FAILURE;
  memcpy(slots, dm->slots.data(), dm->slots.size() * sizeof(unsigned));
  memcpy(lengths, dm->lengths.data(), dm->lengths.size() * sizeof(double));
  return PLL_SUCCESS;
}

PLL_EXPORT pll_utree_t * pllhip_distmat_nj(pllhip_distmat_t * dm, const char * const * labels)
{
  if (!dm || dm->T < 3)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_distmat_nj: no matrix, or fewer than 3 taxa");
    return nullptr;
  }
  if (!dm->joined && !run_nj(dm)) return nullptr;
  return pllhip_nj_build_tree(dm->T, dm->slots.data(), dm->lengths.data(), labels);
}

PLL_EXPORT void pllhip_distances_last_times(double * upload_ms, double * codes_ms, double * counts_ms, double * estimate_ms,
                                            double * nj_ms)
{
  double * out[5] = {upload_ms, codes_ms, counts_ms, estimate_ms, nj_ms};
  for (int k = 0; k < 5; ++k) if (out[k]) *out[k] = g_last_ms[k];
}

}
