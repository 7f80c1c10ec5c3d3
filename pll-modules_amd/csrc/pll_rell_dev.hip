// pll_rell_dev.hip -- site-likelihood sets, RELL resampling with the KH, SH and ELW statistics, bootstrap replicate
// weights (kernels_rell.hpp), and the AU test from multiscale replicates (kernels_au.hpp); contract: INTEGRATION.md,
// "Topology tests and bootstrap weights"; design: DESIGN.md sections 20 and 25.
//
// A set lives on one device, with a stream of its own.  Rows arrive from the host or, device to device, from the
// per-site buffer of an edge log-likelihood (loglikelihood_impl, persite_dev): that copy runs on the engine's stream
// and the set's stream is ordered after it with an event.  pllhip_sitelh_rell works through the replicates in batches
// that bound the memory of the counts; nothing it computes depends on the batch.
#include "device_job.hpp"
#include "kernels_au.hpp"
#include "kernels_rell.hpp"
#include "pllhip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pllhip;

namespace {

using u64 = unsigned long long;

constexpr u64 RELL_MAX_DRAWS = 1ULL << 40;       // the counter keeps 40 bits for the draw ...
constexpr unsigned RELL_MAX_REPLICATES = 1u << 24;   // ... and 24 for the replicate
constexpr unsigned RELL_MAX_BATCH = 16384;       // (also keeps grid.y of the draw kernel legal)
constexpr unsigned RELL_DRAW_MAX_GRID = 1024;
constexpr unsigned RELL_FLAG_MAX_GRID = 2048;
constexpr size_t WEIGHTS_STAGE_BYTES = (size_t)256 << 20;

thread_local double g_last_ms[3] = {0.0, 0.0, 0.0};      // draw, product, statistics of the last call

size_t pad16(size_t n) { return (n + RELL_TILE - 1) / RELL_TILE * RELL_TILE; }

// what the draw kernel searches; all empty for unit weights, where a site is its pattern
struct DrawTable
{
  std::vector<u64> cum;           // [S] inclusive prefix sums of the weights
  std::vector<unsigned> first;    // [buckets + 1]: the pattern of site j << shift; the last entry is S - 1
  unsigned shift = 0;             // the smallest that leaves at most S + 1 buckets
};

// N = sum of the weights, their prefix sums and bucket table; false: N is not in 1 .. 2^40 - 1
bool prefix_sums(const char * who, const unsigned * weights, unsigned S, DrawTable & table, u64 * N)
{
  std::vector<u64> & cum = table.cum;
  bool unit = true;
  u64 sum = 0;
  for (unsigned s = 0; s < S; ++s)
  {
    const unsigned w = weights ? weights[s] : 1u;
    unit = unit && w == 1u;
    sum += w;
  }
  if (!sum || sum >= RELL_MAX_DRAWS)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: the weights add up to %llu (1 to 2^40 - 1 are supported)", who, sum);
    return false;
  }
  *N = sum;
  cum.clear();
  table.first.clear();
  table.shift = 0;
  if (unit) return true;
  cum.resize(S);
  sum = 0;
  for (unsigned s = 0; s < S; ++s) cum[s] = sum += weights[s];
  unsigned shift = 0;
  while (((sum - 1) >> shift) > (u64)S) ++shift;
  const u64 buckets = ((sum - 1) >> shift) + 1;
  table.shift = shift;
  table.first.resize(buckets + 1);
  unsigned s = 0;
  for (u64 j = 0; j < buckets; ++j)
  {
    while (cum[s] <= (j << shift)) ++s;       // (j << shift < N = cum[S - 1])
    table.first[j] = s;
  }
  table.first[buckets] = S - 1;
  return true;
}

// counts of replicates first_b .. first_b + nb - 1 into rows 0 .. nb - 1 of C (cleared here, pad16(nb) rows)
bool draw_batch(hipStream_t stream, const u64 * d_cum, const unsigned * d_first, unsigned shift, size_t Sp, u64 N,
                u64 seed, unsigned first_b, unsigned nb, unsigned * d_C)
{
  if (!hip_ok(hipMemsetAsync(d_C, 0, pad16(nb) * Sp * sizeof(unsigned), stream), "memset counts")) return false;
  const unsigned gx = (unsigned)std::min<u64>((N + RELL_WG - 1) / RELL_WG, RELL_DRAW_MAX_GRID);
  hipLaunchKernelGGL(k_rell_draw, dim3(gx, nb), dim3(RELL_WG), 0, stream, d_cum, d_first, shift, Sp, N, seed,
                     first_b, d_C);
  return hip_ok(hipGetLastError(), "draw kernel");
}

} // namespace

struct pllhip_sitelh
{
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t edge_done = nullptr;     // the last device-to-device row copy on an engine's stream
  unsigned S = 0;
  size_t Sp = 0;                      // row stride of L and of the counts: S padded to 16, the padding is 0
  unsigned count = 0, cap = 0;        // rows in use, rows allocated (a multiple of 16; unused rows are 0)
  double * d_L = nullptr;
  unsigned * d_w = nullptr;           // [Sp]
  u64 * d_cum = nullptr;              // [S], nullptr for unit weights
  unsigned * d_first = nullptr;       // the bucket table of the draws (DrawTable), nullptr for unit weights
  unsigned shift = 0;
  u64 N = 0;
  bool unscanned = false;             // a row was written on the device since the last scan for non-finite values
};

namespace {

bool check_set(const pllhip_sitelh_t * set, const char * who)
{
  if (set) return true;
  set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL set", who);
  return false;
}

// room for `rows` rows; new rows are zero
bool ensure_rows(pllhip_sitelh_t * set, unsigned rows)
{
  if (rows <= set->cap) return true;
  const unsigned cap = (unsigned)pad16(std::max(rows, 2 * set->cap));
  DevBuf<double> d_new;
  const size_t bytes = (size_t)cap * set->Sp * sizeof(double);
  if (!d_new.alloc((size_t)cap * set->Sp, "site likelihoods")) return false;
  const size_t used = (size_t)set->cap * set->Sp * sizeof(double);
  // (every device-to-device row copy so far precedes this on the set's stream: pllhip_sitelh_add_edge)
  if (!hip_ok(hipMemsetAsync(reinterpret_cast<char *>(d_new.p) + used, 0, bytes - used, set->stream), "memset rows") ||
      (used && !hip_ok(hipMemcpyAsync(d_new.p, set->d_L, used, hipMemcpyDeviceToDevice, set->stream), "copy rows")) ||
      !hip_ok(hipStreamSynchronize(set->stream), "copy rows"))
    return false;
  (void)hipFree(set->d_L);
  set->d_L = d_new.release();
  set->cap = cap;
  return true;
}

// product + reduction of the first nb rows of C: R[nb][T]
bool replicate_sums(const pllhip_sitelh_t * set, const unsigned * d_C, unsigned nb, double * d_P, double * d_R)
{
  const unsigned T = set->count, ttiles = (unsigned)(pad16(T) / RELL_TILE), btiles = (unsigned)(pad16(nb) / RELL_TILE);
  const unsigned chunk = rell_chunk_len(set->S), nchunks = (unsigned)((set->Sp + chunk - 1) / chunk);
  hipLaunchKernelGGL(k_rell_product, dim3(nchunks, (btiles + 3) / 4, (ttiles + RELL_TGROUP - 1) / RELL_TGROUP),
                     dim3(RELL_WG), 0, set->stream, d_C, (const double *)set->d_L, set->Sp, chunk, btiles, ttiles, d_P);
  if (!hip_ok(hipGetLastError(), "product kernel")) return false;
  const size_t cells = (size_t)nb * T;
  hipLaunchKernelGGL(k_rell_reduce, dim3((unsigned)((cells + RELL_WG - 1) / RELL_WG)), dim3(RELL_WG), 0, set->stream,
                     (const double *)d_P, nchunks, (size_t)btiles * RELL_TILE, (size_t)ttiles * RELL_TILE, nb, T, d_R);
  return hip_ok(hipGetLastError(), "reduction kernel");
}

// a non-finite value in a row the device wrote: PLL_FAILURE, naming row and pattern
bool scan_rows(pllhip_sitelh_t * set, const char * who)
{
  if (!set->unscanned) return true;
  DevBuf<u64> d_bad;
  u64 bad = ~0ULL;
  if (!d_bad.alloc(1, "the row scan") ||
      !hip_ok(hipMemsetAsync(d_bad.p, 0xff, sizeof(u64), set->stream), "memset scan")) return false;
  const u64 total = (u64)set->count * set->S;
  const unsigned grid = (unsigned)std::min<u64>((total + RELL_WG - 1) / RELL_WG, RELL_FLAG_MAX_GRID);
  hipLaunchKernelGGL(k_rell_flag, dim3(grid), dim3(RELL_WG), 0, set->stream, (const double *)set->d_L, set->count,
                     set->S, set->Sp, d_bad.p);
  if (!hip_ok(hipGetLastError(), "scan kernel") ||
      !hip_ok(hipMemcpyAsync(&bad, d_bad.p, sizeof(u64), hipMemcpyDeviceToHost, set->stream), "download scan") ||
      !hip_ok(hipStreamSynchronize(set->stream), "scan kernel")) return false;
  if (bad != ~0ULL)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: non-finite site log-likelihood in row %llu at pattern %llu", who,
              bad / set->S, bad % set->S);
    return false;
  }
  set->unscanned = false;
  return true;
}

// the observed log-likelihoods, on the device and the host, and the best tree: the weights as the only replicate of a
// batch of their own (d_C holds at least 16 rows)
bool observed_lnl(const pllhip_sitelh_t * set, unsigned * d_C, double * d_P, double * d_lnl, double * lnl, unsigned * best)
{
  const size_t Sp = set->Sp;
  hipStream_t st = set->stream;
  if (!hip_ok(hipMemsetAsync(d_C, 0, RELL_TILE * Sp * sizeof(unsigned), st), "memset counts") ||
      !hip_ok(hipMemcpyAsync(d_C, set->d_w, Sp * sizeof(unsigned), hipMemcpyDeviceToDevice, st), "copy weights") ||
      !replicate_sums(set, d_C, 1, d_P, d_lnl) ||
      !hip_ok(hipMemcpyAsync(lnl, d_lnl, set->count * sizeof(double), hipMemcpyDeviceToHost, st), "download lnl") ||
      !hip_ok(hipStreamSynchronize(st), "observed log-likelihoods"))
    return false;
  *best = 0;
  for (unsigned t = 1; t < set->count; ++t) if (lnl[t] > lnl[*best]) *best = t;
  return true;
}

// replicates per pass when the caller leaves it to the library: what half of the free device memory holds of counts
// (Sp x 4 bytes) and chunk partials (chunks x padded trees x 8 bytes) per replicate
unsigned default_batch(const pllhip_sitelh_t * set, unsigned B)
{
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)1 << 30; }
  const unsigned chunk = rell_chunk_len(set->S), nchunks = (unsigned)((set->Sp + chunk - 1) / chunk);
  const size_t per = set->Sp * sizeof(unsigned) + (size_t)nchunks * pad16(set->count) * sizeof(double);
  const size_t fit = (free_b / 2) / per / RELL_TILE * RELL_TILE;
  return (unsigned)std::max<size_t>(RELL_TILE, std::min<size_t>({fit, RELL_MAX_BATCH, pad16(B)}));
}

bool rell_run(pllhip_sitelh_t * set, const pllhip_rell_params_t * params, pllhip_rell_result_t * res)
{
  const unsigned T = set->count, B = params->replicates, S = set->S;
  const size_t Sp = set->Sp;
  hipStream_t st = set->stream;
  DeviceJob j;                                   // the set's device and stream; the events of the clocks
  if (!j.enter(set->device, st) || !scan_rows(set, "pllhip_sitelh_rell")) return false;
  unsigned batch = params->batch ? (unsigned)std::min<size_t>({pad16(params->batch), RELL_MAX_BATCH, pad16(B)})
                                 : default_batch(set, B);
  res->batch = batch;
  const unsigned chunk = rell_chunk_len(S), nchunks = (unsigned)((Sp + chunk - 1) / chunk);
  const size_t Tp = pad16(T);
  DevBuf<unsigned> d_C, d_cnt;
  DevBuf<double> d_P, d_R, d_E, d_vec;
  if (!d_C.alloc((size_t)batch * Sp, "replicate counts") || !d_P.alloc((size_t)nchunks * batch * Tp, "chunk partials") ||
      !d_R.alloc((size_t)B * T, "replicate log-likelihoods") || !d_E.alloc((size_t)B * T, "likelihood weights") ||
      !d_vec.alloc((size_t)4 * T, "tree statistics") || !d_cnt.alloc((size_t)3 * T, "tree counts"))
    return false;
  double * d_lnl = d_vec.p, * d_meanR = d_vec.p + T, * d_meanD = d_vec.p + 2 * T, * d_elw = d_vec.p + 3 * T;

  unsigned best = 0;
  if (!observed_lnl(set, d_C.p, d_P.p, d_lnl, res->lnl, &best)) return false;
  res->best = best;

  std::vector<hipEvent_t> marks;
  for (unsigned first = 0; first < B; first += batch)
  {
    const unsigned nb = std::min(batch, B - first);
    marks.push_back(j.mark());
    if (!marks.back() || !draw_batch(st, set->d_cum, set->d_first, set->shift, Sp, set->N, params->seed, first, nb, d_C.p)) return false;
    marks.push_back(j.mark());
    if (!marks.back() || !replicate_sums(set, d_C.p, nb, d_P.p, d_R.p + (size_t)first * T)) return false;
  }
  hipEvent_t stats_begin = j.mark();
  if (!stats_begin || !hip_ok(hipMemsetAsync(d_cnt.p, 0, (size_t)3 * T * sizeof(unsigned), st), "memset counts")) return false;
  hipLaunchKernelGGL(k_rell_colmean, dim3(T), dim3(RELL_WG), 0, st, (const double *)d_R.p, B, T, -1, d_meanR);
  hipLaunchKernelGGL(k_rell_colmean, dim3(T), dim3(RELL_WG), 0, st, (const double *)d_R.p, B, T, (int)best, d_meanD);
  hipLaunchKernelGGL(k_rell_counts, dim3(std::min((B + RELL_WG - 1) / RELL_WG, 1024u)), dim3(RELL_WG), 0, st,
                     (const double *)d_R.p, B, T, (const double *)d_lnl, best, (const double *)d_meanR,
                     (const double *)d_meanD, d_cnt.p, d_cnt.p + T, d_cnt.p + 2 * T, d_E.p);
  hipLaunchKernelGGL(k_rell_colmean, dim3(T), dim3(RELL_WG), 0, st, (const double *)d_E.p, B, T, -1, d_elw);
  if (!hip_ok(hipGetLastError(), "statistics kernels")) return false;
  hipEvent_t stats_end = j.mark();
  if (!stats_end ||
      !hip_ok(hipMemcpyAsync(res->bp_count, d_cnt.p, T * sizeof(unsigned), hipMemcpyDeviceToHost, st), "download counts") ||
      !hip_ok(hipMemcpyAsync(res->kh_count, d_cnt.p + T, T * sizeof(unsigned), hipMemcpyDeviceToHost, st), "download counts") ||
      !hip_ok(hipMemcpyAsync(res->sh_count, d_cnt.p + 2 * T, T * sizeof(unsigned), hipMemcpyDeviceToHost, st), "download counts") ||
      !hip_ok(hipMemcpyAsync(res->elw, d_elw, T * sizeof(double), hipMemcpyDeviceToHost, st), "download weights") ||
      (res->replicate_lnl &&
       !hip_ok(hipMemcpyAsync(res->replicate_lnl, d_R.p, (size_t)B * T * sizeof(double), hipMemcpyDeviceToHost, st),
               "download replicates")) ||
      !hip_ok(hipStreamSynchronize(st), "resampling kernels"))
    return false;
  double ms[3] = {0.0, 0.0, 0.0};
  float f = 0.f;
  for (size_t k = 0; k < marks.size(); ++k)
  {
    hipEvent_t next = k + 1 < marks.size() ? marks[k + 1] : stats_begin;
    if (!j.elapsed(marks[k], next, &f)) return false;
    ms[k & 1] += f;
  }
  if (!j.elapsed(stats_begin, stats_end, &f)) return false;
  ms[2] = f;
  for (int k = 0; k < 3; ++k) g_last_ms[k] = ms[k];
  return true;
}

// ---- the AU test: multiscale replicates (kernels_au.hpp) ----

constexpr unsigned AU_MAX_SCALES = 64;
const double AU_DEFAULT_SCALES[10] = {5 / 10.0, 6 / 10.0, 7 / 10.0, 8 / 10.0, 9 / 10.0, 10 / 10.0, 11 / 10.0, 12 / 10.0,
                                      13 / 10.0, 14 / 10.0};

thread_local double g_au_last_ms[3] = {0.0, 0.0, 0.0};   // draw, product, counts + fit of the last call

// n_k = floor(r_k N + 0.5) of every scale; false with the error set: a scale that is not finite and positive, an n_k
// outside 1 .. 2^40 - 1, or two scales of the same n_k
bool au_draw_counts(const double * scale, unsigned K, u64 N, std::vector<u64> & n)
{
  n.assign(K, 0);
  for (unsigned k = 0; k < K; ++k)
  {
    const double r = scale[k];
    if (!std::isfinite(r) || r <= 0.0)
    {
      set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_au: scale %u is %g (finite and positive values are supported)", k, r);
      return false;
    }
    const double x = std::floor(r * (double)N + 0.5);
    if (x < 1.0 || x >= (double)RELL_MAX_DRAWS)
    {
      set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_au: scale %u (%g) of %llu sites draws %.0f (1 to 2^40 - 1 are supported)",
                k, r, N, x);
      return false;
    }
    n[k] = (u64)x;
    for (unsigned i = 0; i < k; ++i)
      if (n[i] == n[k])
      {
        set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_au: scales %u and %u both draw %llu sites", i, k, n[k]);
        return false;
      }
  }
  return true;
}

// rows first .. first + nb - 1 of the K x B rows (scale-major) into rows[0 .. nb - 1]; returns the largest n among them
u64 au_fill_rows(au_row * rows, u64 first, unsigned nb, unsigned B, const std::vector<u64> & seeds,
                 const std::vector<u64> & n)
{
  u64 longest = 0;
  for (unsigned i = 0; i < nb; ++i)
  {
    const unsigned k = (unsigned)((first + i) / B);
    rows[i] = au_row{seeds[k], n[k], (unsigned)((first + i) % B), k};
    longest = std::max(longest, n[k]);
  }
  return longest;
}

// counts of the nb rows the table describes into rows 0 .. nb - 1 of C (cleared here, pad16(nb) rows)
bool au_draw_batch(hipStream_t stream, const u64 * d_cum, const unsigned * d_first, unsigned shift, size_t Sp, u64 N,
                   const au_row * d_rows, unsigned nb, u64 longest, unsigned * d_C)
{
  if (!hip_ok(hipMemsetAsync(d_C, 0, pad16(nb) * Sp * sizeof(unsigned), stream), "memset counts")) return false;
  const unsigned gx = (unsigned)std::min<u64>((longest + RELL_WG - 1) / RELL_WG, RELL_DRAW_MAX_GRID);
  hipLaunchKernelGGL(k_au_draw, dim3(gx, nb), dim3(RELL_WG), 0, stream, d_cum, d_first, shift, Sp, N, d_rows, d_C);
  return hip_ok(hipGetLastError(), "multiscale draw kernel");
}

bool au_run(pllhip_sitelh_t * set, const pllhip_au_params_t * params, const std::vector<u64> & n, pllhip_au_result_t * res)
{
  const unsigned T = set->count, B = params->replicates, K = res->scales, S = set->S;
  const size_t Sp = set->Sp;
  const u64 total = (u64)K * B;                  // rows of R, scale-major (< 2^30)
  hipStream_t st = set->stream;
  DeviceJob j;
  if (!j.enter(set->device, st) || !scan_rows(set, "pllhip_sitelh_au")) return false;
  const unsigned batch = params->batch ? (unsigned)std::min<u64>({pad16(params->batch), RELL_MAX_BATCH, pad16(total)})
                                       : default_batch(set, (unsigned)total);
  res->batch = batch;
  const bool keep = params->flags & PLLHIP_AU_REPLICATES;
  const unsigned chunk = rell_chunk_len(S), nchunks = (unsigned)((Sp + chunk - 1) / chunk);
  unsigned * d_C = j.alloc<unsigned>((size_t)batch * Sp, "replicate counts");
  double * d_P = j.alloc<double>((size_t)nchunks * batch * pad16(T), "chunk partials");
  double * d_R = j.alloc<double>((keep ? total : batch) * T, "replicate log-likelihoods");
  double * d_vec = j.alloc<double>((size_t)6 * T + K, "tree statistics");
  unsigned * d_cnt = j.alloc<unsigned>((size_t)K * T + T, "proportion counts");
  au_row * d_rows = j.alloc<au_row>(batch, "row table");
  au_row * h_rows = j.pinned<au_row>(batch);
  if (!d_C || !d_P || !d_R || !d_vec || !d_cnt || !d_rows || !h_rows) return false;
  double * d_lnl = d_vec, * d_fit = d_vec + T, * d_rho = d_vec + 6 * T;
  unsigned * d_bp = d_cnt, * d_used = d_cnt + (size_t)K * T;

  if (!observed_lnl(set, d_C, d_P, d_lnl, res->lnl, &res->best)) return false;

  std::vector<u64> seeds(K);
  std::vector<double> rho(K);
  unsigned kstar = 0;                            // the scale whose n_k is nearest to N, the lowest on ties
  const u64 N = set->N;
  auto gap = [N](u64 draws) { return draws > N ? draws - N : N - draws; };
  for (unsigned k = 0; k < K; ++k)
  {
    seeds[k] = au_scale_seed(params->seed, k);
    rho[k] = (double)n[k] / (double)N;
    if (gap(n[k]) < gap(n[kstar])) kstar = k;
  }
  if (!j.upload(d_rho, rho.data(), K, "upload scales") ||
      !hip_ok(hipMemsetAsync(d_bp, 0, (size_t)K * T * sizeof(unsigned), st), "memset proportions")) return false;

  std::vector<hipEvent_t> marks;                 // per pass: draw, product, counts
  for (u64 first = 0; first < total; first += batch)
  {
    const unsigned nb = (unsigned)std::min<u64>(batch, total - first);
    // (the pinned table is free again: the pass before has read it)
    if (first && !hip_ok(hipStreamSynchronize(st), "multiscale pass")) return false;
    const u64 longest = au_fill_rows(h_rows, first, nb, B, seeds, n);
    double * d_Rpass = keep ? d_R + first * T : d_R;
    marks.push_back(j.mark());
    if (!marks.back() || !j.upload(d_rows, h_rows, nb, "upload row table") ||
        !au_draw_batch(st, set->d_cum, set->d_first, set->shift, Sp, set->N, d_rows, nb, longest, d_C)) return false;
    marks.push_back(j.mark());
    if (!marks.back() || !replicate_sums(set, d_C, nb, d_P, d_Rpass)) return false;
    marks.push_back(j.mark());
    if (!marks.back()) return false;
    hipLaunchKernelGGL(k_au_counts, dim3((nb + RELL_WG - 1) / RELL_WG), dim3(RELL_WG), 0, st, (const double *)d_Rpass,
                       (const au_row *)d_rows, nb, T, d_bp);
    if (!hip_ok(hipGetLastError(), "proportion kernel")) return false;
  }
  hipEvent_t fit_begin = j.mark();
  if (!fit_begin) return false;
  hipLaunchKernelGGL(k_au_fit, dim3((T + RELL_WG - 1) / RELL_WG), dim3(RELL_WG), 0, st, (const unsigned *)d_bp,
                     (const double *)d_rho, K, T, B, kstar, d_fit, d_fit + T, d_fit + 2 * T, d_fit + 3 * T, d_fit + 4 * T,
                     d_used);
  if (!hip_ok(hipGetLastError(), "fit kernel")) return false;
  hipEvent_t fit_end = j.mark();
  if (!fit_end || !j.download(res->bp_count, d_bp, (size_t)K * T, "download proportions") ||
      !j.download(res->used, d_used, T, "download fit") || !j.download(res->p_au, d_fit, T, "download fit") ||
      !j.download(res->d, d_fit + T, T, "download fit") || !j.download(res->c, d_fit + 2 * T, T, "download fit") ||
      !j.download(res->se, d_fit + 3 * T, T, "download fit") || !j.download(res->rss, d_fit + 4 * T, T, "download fit") ||
      (keep && !j.download(res->replicate_lnl, d_R, total * T, "download replicates")) ||
      !hip_ok(hipStreamSynchronize(st), "multiscale kernels"))
    return false;
  double ms[3] = {0.0, 0.0, 0.0};
  float f = 0.f;
  for (size_t k = 0; k < marks.size(); ++k)
  {
    hipEvent_t next = k + 1 < marks.size() ? marks[k + 1] : fit_begin;
    if (!j.elapsed(marks[k], next, &f)) return false;
    ms[k % 3] += f;
  }
  if (!j.elapsed(fit_begin, fit_end, &f)) return false;
  ms[2] += f;
  for (int k = 0; k < 3; ++k) g_au_last_ms[k] = ms[k];
  return true;
}

} // namespace

extern "C" {

PLL_EXPORT pllhip_sitelh_t * pllhip_sitelh_create(unsigned int patterns, const unsigned int * weights)
{
  if (!patterns)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_create: no patterns");
    return nullptr;
  }
  DrawTable table;
  const std::vector<u64> & cum = table.cum;
  u64 N = 0;
  int device = -1;
  if (!prefix_sums("pllhip_sitelh_create", weights, patterns, table, &N) || !caller_device("pllhip_sitelh_create", &device))
    return nullptr;
  DeviceScope scope;
  if (!scope.enter(device)) return nullptr;
  pllhip_sitelh_t * set = new pllhip_sitelh;
  set->device = device;
  set->S = patterns;
  set->Sp = pad16(patterns);
  set->N = N;
  std::vector<unsigned> w(set->Sp, 0u);
  for (unsigned s = 0; s < patterns; ++s) w[s] = weights ? weights[s] : 1u;
  DevBuf<unsigned> d_w, d_first;
  DevBuf<u64> d_cum;
  const bool ok =
      hip_ok(hipStreamCreateWithFlags(&set->stream, hipStreamNonBlocking), "hipStreamCreate") &&
      hip_ok(hipEventCreateWithFlags(&set->edge_done, hipEventDisableTiming), "hipEventCreate") &&
      d_w.alloc(set->Sp, "pattern weights") &&
      (cum.empty() || (d_cum.alloc(patterns, "weight prefix sums") && d_first.alloc(table.first.size(), "draw buckets"))) &&
      hip_ok(hipMemcpyAsync(d_w.p, w.data(), set->Sp * sizeof(unsigned), hipMemcpyHostToDevice, set->stream),
             "upload weights") &&
      (cum.empty() || hip_ok(hipMemcpyAsync(d_cum.p, cum.data(), (size_t)patterns * sizeof(u64), hipMemcpyHostToDevice,
                                            set->stream), "upload prefix sums")) &&
      (cum.empty() || hip_ok(hipMemcpyAsync(d_first.p, table.first.data(), table.first.size() * sizeof(unsigned),
                                            hipMemcpyHostToDevice, set->stream), "upload draw buckets")) &&
      hip_ok(hipStreamSynchronize(set->stream), "upload weights");
  if (!ok)
  {
    pllhip_sitelh_destroy(set);
    return nullptr;
  }
  set->d_w = d_w.release();
  set->d_cum = d_cum.release();
  set->d_first = d_first.release();
  set->shift = table.shift;
  return set;
}

PLL_EXPORT void pllhip_sitelh_destroy(pllhip_sitelh_t * set)
{
  if (!set) return;
  DeviceScope scope;
  (void)scope.enter(set->device);
  if (set->stream) (void)hipStreamSynchronize(set->stream);
  (void)hipFree(set->d_L);
  (void)hipFree(set->d_w);
  (void)hipFree(set->d_cum);
  (void)hipFree(set->d_first);
  if (set->edge_done) (void)hipEventDestroy(set->edge_done);
  if (set->stream) (void)hipStreamDestroy(set->stream);
  delete set;
}

PLL_EXPORT unsigned int pllhip_sitelh_count(const pllhip_sitelh_t * set) { return set ? set->count : 0; }

PLL_EXPORT int pllhip_sitelh_get(pllhip_sitelh_t * set, unsigned int tree, double * out)
{
  if (!check_set(set, "pllhip_sitelh_get")) return PLL_FAILURE;
  if (tree >= set->count || !out)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_get: row %u of %u, or no output array", tree, set->count);
    return PLL_FAILURE;
  }
  DeviceScope scope;
  if (!scope.enter(set->device)) return PLL_FAILURE;
  PLLHIP_TRY(hipMemcpyAsync(out, set->d_L + (size_t)tree * set->Sp, (size_t)set->S * sizeof(double),
                            hipMemcpyDeviceToHost, set->stream));
  PLLHIP_TRY(hipStreamSynchronize(set->stream));
  return PLL_SUCCESS;
}

PLL_EXPORT int pllhip_sitelh_add(pllhip_sitelh_t * set, const double * row)
{
  if (!check_set(set, "pllhip_sitelh_add")) return -1;
  if (!row)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_add: NULL row");
    return -1;
  }
  for (unsigned s = 0; s < set->S; ++s)
    if (!std::isfinite(row[s]))
    {
      set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_add: non-finite site log-likelihood at pattern %u", s);
      return -1;
    }
  DeviceScope scope;
  if (!scope.enter(set->device) || !ensure_rows(set, set->count + 1) ||
      !hip_ok(hipMemcpyAsync(set->d_L + (size_t)set->count * set->Sp, row, (size_t)set->S * sizeof(double),
                             hipMemcpyHostToDevice, set->stream), "upload row") ||
      !hip_ok(hipStreamSynchronize(set->stream), "upload row"))
    return -1;
  return (int)set->count++;
}

PLL_EXPORT int pllhip_sitelh_add_edge(pllhip_sitelh_t * set, unsigned int tree, unsigned int offset,
                                      pll_partition_t * partition, unsigned int parent_clv_index,
                                      int parent_scaler_index, unsigned int child_clv_index, int child_scaler_index,
                                      unsigned int matrix_index, const unsigned int * freqs_indices, double * lnl)
{
  if (!check_set(set, "pllhip_sitelh_add_edge")) return PLL_FAILURE;
  if (!partition || !partition->engine)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_add_edge: NULL partition");
    return PLL_FAILURE;
  }
  if (tree > set->count)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_add_edge: row %u of a set of %u", tree, set->count);
    return PLL_FAILURE;
  }
  const unsigned sites = partition->sites;
  if ((u64)offset + sites > set->S)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_add_edge: patterns %u .. %llu of %u", offset,
              (u64)offset + sites, set->S);
    return PLL_FAILURE;
  }
  DeviceScope scope;
  if (!scope.enter(set->device) || !ensure_rows(set, tree + 1)) return PLL_FAILURE;
  double * dst = set->d_L + (size_t)tree * set->Sp + offset;
  Engine * e = engine_of(partition);
  double value;
  pll_errno = 0;
  if (is_router(partition) || e->device != set->device)
  {
    std::vector<double> host(sites ? sites : 1);
    value = pll_compute_edge_loglikelihood(partition, parent_clv_index, parent_scaler_index, child_clv_index,
                                           child_scaler_index, matrix_index, freqs_indices, host.data());
    if (pll_errno) return PLL_FAILURE;
    PLLHIP_TRY(hipSetDevice(set->device));
    PLLHIP_TRY(hipMemcpyAsync(dst, host.data(), (size_t)sites * sizeof(double), hipMemcpyHostToDevice, set->stream));
    PLLHIP_TRY(hipStreamSynchronize(set->stream));
  }
  else
  {
    value = loglikelihood_impl(partition, parent_clv_index, parent_scaler_index, child_clv_index, child_scaler_index,
                               (int)matrix_index, freqs_indices, nullptr, nullptr, dst);
    if (pll_errno) return PLL_FAILURE;
    PLLHIP_TRY(hipEventRecord(set->edge_done, e->stream));
    PLLHIP_TRY(hipStreamWaitEvent(set->stream, set->edge_done, 0));
  }
  set->unscanned = true;
  if (tree == set->count) set->count++;
  if (lnl) *lnl = value;
  return PLL_SUCCESS;
}

PLL_EXPORT void pllhip_rell_destroy(pllhip_rell_result_t * result)
{
  if (!result) return;
  free(result->lnl);
  free(result->bp_count);
  free(result->kh_count);
  free(result->sh_count);
  free(result->elw);
  free(result->replicate_lnl);
  free(result);
}

PLL_EXPORT pllhip_rell_result_t * pllhip_sitelh_rell(pllhip_sitelh_t * set, const pllhip_rell_params_t * params)
{
  if (!check_set(set, "pllhip_sitelh_rell")) return nullptr;
  if (!params || !params->replicates || params->replicates >= RELL_MAX_REPLICATES)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_rell: %u replicates (1 to 2^24 - 1 are supported)",
              params ? params->replicates : 0u);
    return nullptr;
  }
  if (!set->count)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_rell: the set holds no tree");
    return nullptr;
  }
  const unsigned T = set->count, B = params->replicates;
  pllhip_rell_result_t * res = (pllhip_rell_result_t *)calloc(1, sizeof(pllhip_rell_result_t));
  if (res)
  {
    res->trees = T;
    res->replicates = B;
    res->lnl = (double *)calloc(T, sizeof(double));
    res->bp_count = (unsigned *)calloc(T, sizeof(unsigned));
    res->kh_count = (unsigned *)calloc(T, sizeof(unsigned));
    res->sh_count = (unsigned *)calloc(T, sizeof(unsigned));
    res->elw = (double *)calloc(T, sizeof(double));
    if (params->flags & PLLHIP_RELL_REPLICATES) res->replicate_lnl = (double *)calloc((size_t)B * T, sizeof(double));
  }
  if (!res || !res->lnl || !res->bp_count || !res->kh_count || !res->sh_count || !res->elw ||
      ((params->flags & PLLHIP_RELL_REPLICATES) && !res->replicate_lnl))
  {
    pllhip_rell_destroy(res);
    set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate memory for the resampling result");
    return nullptr;
  }
  if (!rell_run(set, params, res))
  {
    pllhip_rell_destroy(res);
    return nullptr;
  }
  return res;
}

PLL_EXPORT void pllhip_rell_last_times(double * draw_ms, double * product_ms, double * stats_ms)
{
  if (draw_ms) *draw_ms = g_last_ms[0];
  if (product_ms) *product_ms = g_last_ms[1];
  if (stats_ms) *stats_ms = g_last_ms[2];
}

PLL_EXPORT int pllhip_bootstrap_weights(const unsigned int * weights, unsigned int patterns, unsigned long long seed,
                                        unsigned int first, unsigned int count, unsigned int * out)
{
  if (!patterns || !out || (u64)first + count > RELL_MAX_REPLICATES - 1)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_bootstrap_weights: no patterns, no output array, or replicates beyond 2^24 - 2");
    return PLL_FAILURE;
  }
  DrawTable table;
  const std::vector<u64> & cum = table.cum;
  u64 N = 0;
  int device = -1;
  if (!prefix_sums("pllhip_bootstrap_weights", weights, patterns, table, &N) ||
      !caller_device("pllhip_bootstrap_weights", &device))
    return PLL_FAILURE;
  if (!count) return PLL_SUCCESS;
  const size_t Sp = pad16(patterns);
  const unsigned batch = (unsigned)std::max<size_t>(
      1, std::min<size_t>({count, RELL_MAX_BATCH, WEIGHTS_STAGE_BYTES / (Sp * sizeof(unsigned))}));
  DeviceJob j;
  DevBuf<unsigned> d_C, d_first;
  DevBuf<u64> d_cum;
  if (!j.enter(device) || !d_C.alloc(pad16(batch) * Sp, "replicate counts") ||
      (!cum.empty() && (!d_cum.alloc(patterns, "weight prefix sums") || !d_first.alloc(table.first.size(), "draw buckets"))))
    return PLL_FAILURE;
  if (!cum.empty())
  {
    PLLHIP_TRY(hipMemcpyAsync(d_cum.p, cum.data(), (size_t)patterns * sizeof(u64), hipMemcpyHostToDevice, j.stream));
    PLLHIP_TRY(hipMemcpyAsync(d_first.p, table.first.data(), table.first.size() * sizeof(unsigned), hipMemcpyHostToDevice,
                              j.stream));
  }
  for (unsigned done = 0; done < count; done += batch)
  {
    const unsigned nb = std::min(batch, count - done);
    if (!draw_batch(j.stream, d_cum.p, d_first.p, table.shift, Sp, N, seed, first + done, nb, d_C.p)) return PLL_FAILURE;
    PLLHIP_TRY(hipMemcpy2DAsync(out + (size_t)done * patterns, (size_t)patterns * sizeof(unsigned), d_C.p,
                                Sp * sizeof(unsigned), (size_t)patterns * sizeof(unsigned), nb, hipMemcpyDeviceToHost,
                                j.stream));
    PLLHIP_TRY(hipStreamSynchronize(j.stream));
  }
  return PLL_SUCCESS;
}

PLL_EXPORT void pllhip_au_destroy(pllhip_au_result_t * result)
{
  if (!result) return;
  free(result->lnl);
  free(result->draws);
  free(result->bp_count);
  free(result->p_au);
  free(result->d);
  free(result->c);
  free(result->se);
  free(result->rss);
  free(result->used);
  free(result->replicate_lnl);
  free(result);
}

PLL_EXPORT pllhip_au_result_t * pllhip_sitelh_au(pllhip_sitelh_t * set, const pllhip_au_params_t * params)
{
  if (!check_set(set, "pllhip_sitelh_au")) return nullptr;
  if (!params || !params->replicates || params->replicates >= RELL_MAX_REPLICATES)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_au: %u replicates per scale (1 to 2^24 - 1 are supported)",
              params ? params->replicates : 0u);
    return nullptr;
  }
  const unsigned K = params->scale ? params->scales : 10u;
  if (K < 2 || K > AU_MAX_SCALES)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_au: %u scales (2 to %u are supported)", K, AU_MAX_SCALES);
    return nullptr;
  }
  if (!set->count)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_sitelh_au: the set holds no tree");
    return nullptr;
  }
  std::vector<u64> n;
  if (!au_draw_counts(params->scale ? params->scale : AU_DEFAULT_SCALES, K, set->N, n)) return nullptr;
  const unsigned T = set->count, B = params->replicates;
  const bool keep = params->flags & PLLHIP_AU_REPLICATES;
  pllhip_au_result_t * res = (pllhip_au_result_t *)calloc(1, sizeof(pllhip_au_result_t));
  if (res)
  {
    res->trees = T;
    res->replicates = B;
    res->scales = K;
    res->lnl = (double *)calloc(T, sizeof(double));
    res->draws = (u64 *)calloc(K, sizeof(u64));
    res->bp_count = (unsigned *)calloc((size_t)K * T, sizeof(unsigned));
    res->p_au = (double *)calloc(T, sizeof(double));
    res->d = (double *)calloc(T, sizeof(double));
    res->c = (double *)calloc(T, sizeof(double));
    res->se = (double *)calloc(T, sizeof(double));
    res->rss = (double *)calloc(T, sizeof(double));
    res->used = (unsigned *)calloc(T, sizeof(unsigned));
    if (keep) res->replicate_lnl = (double *)calloc((size_t)K * B * T, sizeof(double));
  }
  if (!res || !res->lnl || !res->draws || !res->bp_count || !res->p_au || !res->d || !res->c || !res->se || !res->rss ||
      !res->used || (keep && !res->replicate_lnl))
  {
    pllhip_au_destroy(res);
    set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate memory for the AU test's result");
    return nullptr;
  }
  std::copy(n.begin(), n.end(), res->draws);
  if (!au_run(set, params, n, res))
  {
    pllhip_au_destroy(res);
    return nullptr;
  }
  return res;
}

PLL_EXPORT void pllhip_au_last_times(double * draw_ms, double * product_ms, double * stats_ms)
{
  if (draw_ms) *draw_ms = g_au_last_ms[0];
  if (product_ms) *product_ms = g_au_last_ms[1];
  if (stats_ms) *stats_ms = g_au_last_ms[2];
}

PLL_EXPORT int pllhip_multiscale_weights(const unsigned int * weights, unsigned int patterns, unsigned long long seed,
                                         unsigned int scale_index, unsigned long long draws, unsigned int first,
                                         unsigned int count, unsigned int * out)
{
  if (!patterns || !out || (u64)first + count > RELL_MAX_REPLICATES - 1 || scale_index >= AU_MAX_SCALES || !draws ||
      draws >= RELL_MAX_DRAWS)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_multiscale_weights: no patterns, no output array, replicates beyond "
              "2^24 - 2, a scale index beyond 63, or draws outside 1 .. 2^40 - 1");
    return PLL_FAILURE;
  }
  DrawTable table;
  const std::vector<u64> & cum = table.cum;
  u64 N = 0;
  int device = -1;
  if (!prefix_sums("pllhip_multiscale_weights", weights, patterns, table, &N) ||
      !caller_device("pllhip_multiscale_weights", &device))
    return PLL_FAILURE;
  if (!count) return PLL_SUCCESS;
  const size_t Sp = pad16(patterns);
  const unsigned batch = (unsigned)std::max<size_t>(
      1, std::min<size_t>({count, RELL_MAX_BATCH, WEIGHTS_STAGE_BYTES / (Sp * sizeof(unsigned))}));
  DeviceJob j;
  if (!j.enter(device)) return PLL_FAILURE;
  unsigned * d_C = j.alloc<unsigned>(pad16(batch) * Sp, "replicate counts");
  au_row * d_rows = j.alloc<au_row>(batch, "row table");
  au_row * h_rows = j.pinned<au_row>(batch);
  u64 * d_cum = cum.empty() ? nullptr : j.alloc<u64>(patterns, "weight prefix sums");
  unsigned * d_first = cum.empty() ? nullptr : j.alloc<unsigned>(table.first.size(), "draw buckets");
  if (!d_C || !d_rows || !h_rows || (!cum.empty() && (!d_cum || !d_first))) return PLL_FAILURE;
  if (!cum.empty() && (!j.upload(d_cum, cum.data(), patterns, "upload prefix sums") ||
                       !j.upload(d_first, table.first.data(), table.first.size(), "upload draw buckets")))
    return PLL_FAILURE;
  const u64 stream_seed = au_scale_seed(seed, scale_index);
  for (unsigned done = 0; done < count; done += batch)
  {
    const unsigned nb = std::min(batch, count - done);
    for (unsigned i = 0; i < nb; ++i) h_rows[i] = au_row{stream_seed, draws, first + done + i, scale_index};
    if (!j.upload(d_rows, h_rows, nb, "upload row table") ||
        !au_draw_batch(j.stream, d_cum, d_first, table.shift, Sp, N, d_rows, nb, draws, d_C))
      return PLL_FAILURE;
    PLLHIP_TRY(hipMemcpy2DAsync(out + (size_t)done * patterns, (size_t)patterns * sizeof(unsigned), d_C,
                                Sp * sizeof(unsigned), (size_t)patterns * sizeof(unsigned), nb, hipMemcpyDeviceToHost,
                                j.stream));
    PLLHIP_TRY(hipStreamSynchronize(j.stream));
  }
  return PLL_SUCCESS;
}

}
