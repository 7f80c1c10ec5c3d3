// pll_msa_stats_dev.hip -- empirical frequencies, exchangeabilities, p-inv and alignment statistics from tips that
// live on the device (kernels_msa_stats.hpp; contract: INTEGRATION.md, "Empirical parameters and alignment
// statistics"; design: DESIGN.md section 15).
//
// The device fills 64-bit integer tables in one pass over the tips; this file makes the few divisions.  The
// partition forms run on the partition's stream (per shard on the shard's device, tables added here); the alignment
// form runs on a stream of its own on the device pllhip_get_device() names.  Everything a call allocates is gone
// when it returns, and nothing of the caller's is written.
#include "device_job.hpp"
#include "kernels_msa_stats.hpp"
#include "msa_upload.hpp"
#include "pllhip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

using namespace pllhip;

namespace {

using u64 = unsigned long long;

constexpr size_t STATS_STAGE_BYTES = (size_t)16 << 20;        // one half of the staging buffer
constexpr unsigned STATS_MAX_GRID = 2048;
constexpr unsigned VECFREQ_MAX_GRID = 1024;

thread_local double g_last_ms[2] = {0.0, 0.0};                // upload, kernels of the last call

unsigned tables_grid(unsigned N, unsigned vpl)
{
  const unsigned tile = MST_WG * vpl;
  return std::max(1u, std::min((N + tile - 1) / tile, STATS_MAX_GRID));
}

// the tier of the state loop: <= 4, <= 32, <= 64 states; coded tips of the first tier take 4 sites per lane
template <bool CODED>
void launch_tables(hipStream_t stream, const TipView & tp, const u64 * d_tipmap, const unsigned * d_weights, unsigned T,
                   unsigned N, unsigned S, u64 * d_tab, uint8_t * d_flags, u64 * d_seq_gap)
{
  if (S <= 4)
  {
    constexpr int VPL = CODED ? 4 : 1;
    hipLaunchKernelGGL((k_mst_tables<4, VPL, CODED>), dim3(tables_grid(N, VPL)), dim3(MST_WG), 0, stream, tp, d_tipmap,
                       d_weights, T, N, S, d_tab, d_flags, d_seq_gap);
  }
  else if (S <= 32)
    hipLaunchKernelGGL((k_mst_tables<32, 1, CODED>), dim3(tables_grid(N, 1)), dim3(MST_WG), 0, stream, tp, d_tipmap,
                       d_weights, T, N, S, d_tab, d_flags, d_seq_gap);
  else
    hipLaunchKernelGGL((k_mst_tables<64, 1, CODED>), dim3(tables_grid(N, 1)), dim3(MST_WG), 0, stream, tp, d_tipmap,
                       d_weights, T, N, S, d_tab, d_flags, d_seq_gap);
}

// lanes per character of k_mst_vecfreq: the power of two >= S
unsigned vecfreq_lanes(unsigned S)
{
  unsigned kp = 2;
  while (kp < S) kp <<= 1;
  return kp;
}

bool clear_tables(u64 * d_tab, hipStream_t stream)
{
  return hip_ok(hipMemsetAsync(d_tab, 0, MST_WORDS * sizeof(u64), stream), "memset tables") &&
         hip_ok(hipMemsetAsync(d_tab + MST_BAD, 0xff, sizeof(u64), stream), "memset tables");
}

// ---------------------------------------------------------------------------------------------------------------
// partition forms
// ---------------------------------------------------------------------------------------------------------------
struct TipTables
{
  DevBuf<const double *> clv;
  DevBuf<const uint8_t *> codes;
  TipView view = {};
};

bool tip_tables(Engine * e, TipTables & tt)
{
  if (!tip_pointer_tables(e, tt.clv, tt.codes)) return false;
  tt.view.code_rows = tt.codes.p;
  tt.view.code_base = nullptr;
  tt.view.code_stride = 0;
  tt.view.clv_rows = tt.clv.p;
  tt.view.R = e->R;
  tt.view.Sp = e->Sp;
  tt.view.brows = e->rows;
  return true;
}

// the integer tables of one ordinary partition (a shard, or the partition itself), added to tab[MST_WORDS]
int add_tables(pll_partition_t * p, std::vector<u64> & tab, double & kernel_ms)
{
  Engine * e = engine_of(p);
  DeviceJob j;
  if (!j.enter(e->device, e->stream) || !upload_tipmap(p)) return PLL_FAILURE;
  TipTables tt;
  u64 * d_tab = j.alloc<u64>(MST_WORDS, "statistics tables");
  hipEvent_t a = j.event(), b = j.event();
  std::vector<u64> h_tab(MST_WORDS);
  if (!tip_tables(e, tt) || !d_tab || !a || !b || !clear_tables(d_tab, e->stream)) return PLL_FAILURE;
  PLLHIP_TRY(hipEventRecord(a, e->stream));
  if (e->coded_tips)
    launch_tables<true>(e->stream, tt.view, e->d_tipmap, e->d_weights, e->tips, e->Nreal, e->S, d_tab, nullptr, nullptr);
  else
    launch_tables<false>(e->stream, tt.view, nullptr, e->d_weights, e->tips, e->Nreal, e->S, d_tab, nullptr, nullptr);
  PLLHIP_TRY(hipGetLastError());
  PLLHIP_TRY(hipEventRecord(b, e->stream));
  float ms = 0.f;
  if (!j.download(h_tab.data(), d_tab, MST_WORDS, "download tables") ||
      !hip_ok(hipStreamSynchronize(e->stream), "statistics kernel") || !j.elapsed(a, b, &ms))
    return PLL_FAILURE;
  kernel_ms += ms;
  for (unsigned i = 1; i < MST_WORDS; ++i) tab[i] += h_tab[i];
  return PLL_SUCCESS;
}

// the floating-point sums of one ordinary partition, its workgroups' partials added to fsum[S] in index order
int add_vecfreq(pll_partition_t * p, std::vector<double> & fsum, double & kernel_ms)
{
  Engine * e = engine_of(p);
  const unsigned kp = vecfreq_lanes(e->S), per_block = MST_WG / kp;
  const unsigned grid = std::max(1u, std::min((e->Nreal + per_block - 1) / per_block, VECFREQ_MAX_GRID));
  DeviceJob j;
  if (!j.enter(e->device, e->stream)) return PLL_FAILURE;
  TipTables tt;
  std::vector<double> h_partial((size_t)grid * e->S);
  double * d_partial = j.alloc<double>(h_partial.size(), "frequency partials");
  hipEvent_t a = j.event(), b = j.event();
  if (!tip_tables(e, tt) || !d_partial || !a || !b) return PLL_FAILURE;
  PLLHIP_TRY(hipEventRecord(a, e->stream));
  hipLaunchKernelGGL(k_mst_vecfreq, dim3(grid), dim3(MST_WG), 0, e->stream, tt.view, (const unsigned *)e->d_weights,
                     e->tips, e->Nreal, e->S, kp, d_partial);
  PLLHIP_TRY(hipGetLastError());
  PLLHIP_TRY(hipEventRecord(b, e->stream));
  float ms = 0.f;
  if (!j.download(h_partial.data(), d_partial, h_partial.size(), "download partials") ||
      !hip_ok(hipStreamSynchronize(e->stream), "frequency kernel") || !j.elapsed(a, b, &ms))
    return PLL_FAILURE;
  kernel_ms += ms;
  for (unsigned b = 0; b < grid; ++b)
    for (unsigned k = 0; k < e->S; ++k) fsum[k] += h_partial[(size_t)b * e->S + k];
  return PLL_SUCCESS;
}

bool check_partition(const pll_partition_t * p, const char * who)
{
  if (!p || !p->engine)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL partition", who);
    return false;
  }
  if (p->states < 2 || p->states > MST_MAX_STATES)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "%s: %u states (2 to %u are supported)", who, p->states, MST_MAX_STATES);
    return false;
  }
  return true;
}

// every shard's tables (in shard order), or the partition's own
int partition_tables(pll_partition_t * p, std::vector<u64> & tab)
{
  Engine * e = engine_of(p);
  double ms = 0.0;
  int rc = PLL_SUCCESS;
  if (e->shards.empty()) rc = add_tables(p, tab, ms);
  else
    for (size_t k = 0; rc && k < e->shards.size(); ++k) rc = add_tables(e->shards[k], tab, ms);
  if (rc) { g_last_ms[0] = 0.0; g_last_ms[1] = ms; }
  return rc;
}

int partition_vecfreq(pll_partition_t * p, std::vector<double> & fsum)
{
  Engine * e = engine_of(p);
  double ms = 0.0;
  int rc = PLL_SUCCESS;
  if (e->shards.empty()) rc = add_vecfreq(p, fsum, ms);
  else
    for (size_t k = 0; rc && k < e->shards.size(); ++k) rc = add_vecfreq(e->shards[k], fsum, ms);
  if (rc) g_last_ms[1] += ms;
  return rc;
}

// ---------------------------------------------------------------------------------------------------------------
// the divisions
// ---------------------------------------------------------------------------------------------------------------
// freq[k] = (sum over c of A[k][c] / c) / total, A[k][c] = weight of the characters that contain k and have c states:
// c = 1 from the diagonal less the ambiguous ones, 1 < c < S from the ambiguity table, c = S (gaps) only where the
// form counts them.  long double, ascending c, rounded once.
void finish_frequencies(const std::vector<u64> & tab, unsigned S, bool with_gaps, u64 total, double * freq)
{
  for (unsigned k = 0; k < S; ++k)
  {
    const u64 * A = tab.data() + MST_AMBIG + (size_t)k * (MST_MAX_STATES + 1);
    u64 ambiguous = 0;
    for (unsigned c = 2; c < S; ++c) ambiguous += A[c];
    long double sum = (long double)(tab[MST_DIAG + k] - ambiguous);
    for (unsigned c = 2; c < S; ++c)
      if (A[c]) sum += (long double)A[c] / (long double)c;
    if (with_gaps) sum += (long double)tab[MST_GAPW] / (long double)S;
    freq[k] = (double)(sum / (long double)total);
  }
}

// pll_msa.c:264-279 on the pair table
void finish_rates(const std::vector<u64> & tab, unsigned S, double * rates)
{
  const unsigned npairs = S * (S - 1) / 2;
  double last_rate = (double)tab[MST_PAIR + npairs - 1];
  if (last_rate < 1e-7) last_rate = 1;
  for (unsigned k = 0; k < npairs; ++k)
  {
    rates[k] = (double)tab[MST_PAIR + k] / last_rate;
    if (rates[k] < 0.01) rates[k] = 0.01;
    if (rates[k] > 50.0) rates[k] = 50.0;
  }
  rates[npairs - 1] = 1.0;
}

// ---------------------------------------------------------------------------------------------------------------
// alignment form
// ---------------------------------------------------------------------------------------------------------------
// pairs (first occurrence, later copy) of equal strings, ordered by first occurrence, then by copy: one hashing pass
bool find_duplicates(char ** strings, size_t count, size_t length, unsigned long ** pairs, unsigned long * npairs)
{
  std::unordered_map<std::string, unsigned long> first;
  std::vector<std::pair<unsigned long, unsigned long>> found;
  first.reserve(count * 2);
  for (size_t i = 0; i < count; ++i)
  {
    std::string key = length ? std::string(strings[i], strnlen(strings[i], length)) : std::string(strings[i]);
    auto it = first.find(key);
    if (it == first.end()) first.emplace(std::move(key), (unsigned long)i);
    else found.emplace_back(it->second, (unsigned long)i);
  }
  std::sort(found.begin(), found.end());
  *npairs = found.size();
  *pairs = nullptr;
  if (found.empty()) return true;
  *pairs = (unsigned long *)malloc(found.size() * 2 * sizeof(unsigned long));
  if (!*pairs)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate memory for duplicates array");
    return false;
  }
  for (size_t k = 0; k < found.size(); ++k) { (*pairs)[2 * k] = found[k].first; (*pairs)[2 * k + 1] = found[k].second; }
  return true;
}

// the device part of the alignment form: tab[MST_WORDS], flags[L], seq_gap[T]
// (want_flags / want_seq_gap: only a mask that asks for them pays for the per-site flags and the per-sequence sums)
bool alignment_tables(const pll_msa_t * msa, unsigned states, const pll_state_t * tipmap, const unsigned * weights,
                      bool want_flags, bool want_seq_gap, std::vector<u64> & tab, std::vector<uint8_t> & flags,
                      std::vector<u64> & seq_gap)
{
  int device = -1;
  if (!caller_device("pllhip_msa_compute_stats", &device)) return false;
  const unsigned T = (unsigned)msa->count, L = (unsigned)msa->length;
  const size_t Lp = ((size_t)L + 255u) & ~(size_t)255u;
  const size_t half = std::min(STATS_STAGE_BYTES, (size_t)T * Lp);
  DeviceJob j;
  MsaStager stager;
  if (!j.enter(device)) return false;
  hipEvent_t ev[3];                                           // start, uploaded, computed
  for (hipEvent_t & e : ev) if (!(e = j.event())) return false;
  uint8_t * d_in = j.alloc<uint8_t>((size_t)T * Lp, "the alignment");
  uint8_t * d_flags = j.alloc<uint8_t>((size_t)L, "column flags");
  u64 * d_map = j.alloc<u64>(256, "the character map");
  u64 * d_tab = j.alloc<u64>(MST_WORDS, "statistics tables");
  u64 * d_seq_gap = j.alloc<u64>((size_t)T, "sequence gap weights");
  unsigned * d_weights = weights ? j.alloc<unsigned>((size_t)L, "column weights") : nullptr;
  if (!d_in || !d_flags || !d_map || !d_tab || !d_seq_gap || (weights && !d_weights) || !stager.open(half)) return false;
  if (!hip_ok(hipEventRecord(ev[0], j.stream), "hipEventRecord") ||
      !stager.rows(j.stream, d_in, msa->sequence, T, L, Lp, half) ||
      !j.upload(d_map, (const u64 *)tipmap, 256, "upload map") ||
      (weights && !j.upload(d_weights, weights, (size_t)L, "upload weights")) || !clear_tables(d_tab, j.stream) ||
      !hip_ok(hipMemsetAsync(d_seq_gap, 0, (size_t)T * sizeof(u64), j.stream), "memset gap weights") ||
      !hip_ok(hipEventRecord(ev[1], j.stream), "hipEventRecord"))
    return false;
  TipView tp = {};
  tp.code_base = d_in;
  tp.code_stride = Lp;
  launch_tables<true>(j.stream, tp, d_map, d_weights, T, L, states, d_tab, want_flags ? d_flags : nullptr,
                      want_seq_gap ? d_seq_gap : nullptr);
  if (!hip_ok(hipGetLastError(), "statistics kernel") || !hip_ok(hipEventRecord(ev[2], j.stream), "hipEventRecord") ||
      !j.download(tab.data(), d_tab, MST_WORDS, "download tables") ||
      (want_flags && !j.download(flags.data(), d_flags, (size_t)L, "download flags")) ||
      (want_seq_gap && !j.download(seq_gap.data(), d_seq_gap, (size_t)T, "download gap weights")) ||
      !hip_ok(hipStreamSynchronize(j.stream), "statistics kernel"))
    return false;
  float up = 0.f, kern = 0.f;
  if (!j.elapsed(ev[0], ev[1], &up) || !j.elapsed(ev[1], ev[2], &kern)) return false;
  g_last_ms[0] = up;
  g_last_ms[1] = kern;
  return true;
}

// indices i < n with keep(i), ascending; *out stays NULL when there are none
template <typename F>
bool index_list(size_t n, F keep, unsigned long ** out, unsigned long * count)
{
  size_t c = 0;
  for (size_t i = 0; i < n; ++i) c += keep(i) ? 1 : 0;
  *count = (unsigned long)c;
  *out = nullptr;
  if (!c) return true;
  *out = (unsigned long *)malloc(c * sizeof(unsigned long));
  if (!*out)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate memory for MSA statistics");
    return false;
  }
  c = 0;
  for (size_t i = 0; i < n; ++i) if (keep(i)) (*out)[c++] = (unsigned long)i;
  return true;
}

} // namespace

extern "C" {

PLL_EXPORT double * pllhip_empirical_frequencies(pll_partition_t * partition)
{
  if (!check_partition(partition, "pllhip_empirical_frequencies")) return nullptr;
  const unsigned S = partition->states;
  std::vector<u64> tab(MST_WORDS, 0);
  if (!partition_tables(partition, tab)) return nullptr;
  const u64 total = tab[MST_WSUM] * partition->tips;
  std::vector<double> fsum(S, 0.0);
  const bool floating = tab[MST_NONBIN] != 0;
  if (floating && !partition_vecfreq(partition, fsum)) return nullptr;
  double * freq = (double *)calloc(S, sizeof(double));
  if (!freq)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate memory for empirical frequencies");
    return nullptr;
  }
  if (floating)
    for (unsigned k = 0; k < S; ++k) freq[k] = fsum[k] / (double)total;
  else
    finish_frequencies(tab, S, true, total, freq);
  return freq;
}

PLL_EXPORT double * pllhip_empirical_subst_rates(pll_partition_t * partition)
{
  if (!check_partition(partition, "pllhip_empirical_subst_rates")) return nullptr;
  const unsigned S = partition->states;
  std::vector<u64> tab(MST_WORDS, 0);
  if (!partition_tables(partition, tab)) return nullptr;
  double * rates = (double *)calloc((size_t)S * (S - 1) / 2, sizeof(double));
  if (!rates)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate memory for empirical subst rates");
    return nullptr;
  }
  finish_rates(tab, S, rates);
  return rates;
}

PLL_EXPORT double pllhip_empirical_invariant_sites(pll_partition_t * partition)
{
  if (!check_partition(partition, "pllhip_empirical_invariant_sites")) return (double)-INFINITY;
  pll_errno = 0;
  if (!partition->invariant && !pll_update_invariant_sites(partition)) return (double)-INFINITY;
  u64 inv = 0, all = 0;
  for (unsigned n = 0; n < partition->sites; ++n)
  {
    if (partition->invariant[n] > -1) inv += partition->pattern_weights[n];
    all += partition->pattern_weights[n];
  }
  return (double)inv / (double)all;
}

PLL_EXPORT void pllhip_msa_destroy_stats(pllhip_msa_stats_t * stats)
{
  if (!stats) return;
  free(stats->dup_taxa_pairs);
  free(stats->dup_seqs_pairs);
  free(stats->gap_seqs);
  free(stats->gap_cols);
  free(stats->inv_cols);
  free(stats->freqs);
  free(stats->subst_rates);
  free(stats);
}

PLL_EXPORT pllhip_msa_stats_t * pllhip_msa_compute_stats(const pll_msa_t * msa, unsigned int states,
                                                         const pll_state_t * tipmap, const unsigned int * weights,
                                                         unsigned long stats_mask)
{
  if (!msa || !tipmap)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_msa_compute_stats: %s is NULL",
              msa ? "Character-to-state mapping" : "MSA structure");
    return nullptr;
  }
  if (states < 2 || states > MST_MAX_STATES)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_msa_compute_stats: %u states (2 to %u are supported)", states,
              MST_MAX_STATES);
    return nullptr;
  }
  if (msa->count < 1 || msa->length < 1 || !msa->sequence || ((stats_mask & PLLHIP_MSA_STATS_DUP_TAXA) && !msa->label))
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pllhip_msa_compute_stats: no sequence, no site, or no labels to compare");
    return nullptr;
  }
  for (int t = 0; t < msa->count; ++t)
    if (!msa->sequence[t] || ((stats_mask & PLLHIP_MSA_STATS_DUP_TAXA) && !msa->label[t]))
    {
      set_error(PLL_ERROR_PARAM_INVALID, "pllhip_msa_compute_stats: sequence or label %d is NULL", t);
      return nullptr;
    }
  const unsigned T = (unsigned)msa->count, L = (unsigned)msa->length, S = states;
  pllhip_msa_stats_t * stats = (pllhip_msa_stats_t *)calloc(1, sizeof(pllhip_msa_stats_t));
  if (!stats)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate memory for MSA statistics");
    return nullptr;
  }
  stats->states = states;
  bool ok = true;
  if (stats_mask & PLLHIP_MSA_STATS_DUP_TAXA)
    ok = find_duplicates(msa->label, T, 0, &stats->dup_taxa_pairs, &stats->dup_taxa_pairs_count);
  if (ok && (stats_mask & PLLHIP_MSA_STATS_DUP_SEQS))
    ok = find_duplicates(msa->sequence, T, L, &stats->dup_seqs_pairs, &stats->dup_seqs_pairs_count);
  if (!ok) { pllhip_msa_destroy_stats(stats); return nullptr; }
  // duplicates only: host work, no device
  if (!(stats_mask & ~(unsigned long)(PLLHIP_MSA_STATS_DUP_TAXA | PLLHIP_MSA_STATS_DUP_SEQS))) return stats;

  std::vector<u64> tab(MST_WORDS, 0), seq_gap(T, 0);
  std::vector<uint8_t> flags(L, 0);
  const bool want_flags =
      (stats_mask & (PLLHIP_MSA_STATS_GAP_COLS | PLLHIP_MSA_STATS_INV_COLS | PLLHIP_MSA_STATS_INV_PROP)) != 0;
  const bool want_seq_gap = (stats_mask & PLLHIP_MSA_STATS_GAP_SEQS) != 0;
  if (!alignment_tables(msa, S, tipmap, weights, want_flags, want_seq_gap, tab, flags, seq_gap))
  {
    pllhip_msa_destroy_stats(stats);
    return nullptr;
  }
  if (tab[MST_BAD] != MST_NO_BAD)
  {
    const u64 t = tab[MST_BAD] / L, s = tab[MST_BAD] % L;
    const char c = msa->sequence[t][s];
    if (c == (char)-1)
      set_error(PLL_ERROR_MSA_MAP_INVALID, "Unknown state in sequence %llu", t + 1);
    else
      set_error(PLL_ERROR_MSA_MAP_INVALID, "Unknown state %c at sequence %llu position %llu", c, t + 1, s + 1);
    pllhip_msa_destroy_stats(stats);
    return nullptr;
  }
  const u64 sum_weights = tab[MST_WSUM], gap_weight = tab[MST_GAPW], total_chars = sum_weights * T;
  if (stats_mask & PLLHIP_MSA_STATS_SUBST_RATES)
  {
    stats->subst_rates = (double *)calloc((size_t)S * (S - 1) / 2, sizeof(double));
    if (stats->subst_rates) finish_rates(tab, S, stats->subst_rates);
    else { set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate memory for MSA statistics"); ok = false; }
  }
  if (ok && (stats_mask & PLLHIP_MSA_STATS_FREQS))
  {
    stats->freqs = (double *)calloc(S, sizeof(double));
    if (stats->freqs) finish_frequencies(tab, S, false, total_chars - gap_weight, stats->freqs);
    else { set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate memory for empirical frequencies"); ok = false; }
  }
  if (stats_mask & PLLHIP_MSA_STATS_GAP_PROP) stats->gap_prop = (double)gap_weight / (double)total_chars;
  if (ok && (stats_mask & PLLHIP_MSA_STATS_GAP_COLS))
    ok = index_list(L, [&](size_t i) { return (flags[i] & MST_FLAG_GAPCOL) != 0; }, &stats->gap_cols, &stats->gap_cols_count);
  if (ok && (stats_mask & PLLHIP_MSA_STATS_GAP_SEQS))
    ok = index_list(T, [&](size_t i) { return seq_gap[i] == sum_weights; }, &stats->gap_seqs, &stats->gap_seqs_count);
  if (ok && (stats_mask & (PLLHIP_MSA_STATS_INV_COLS | PLLHIP_MSA_STATS_INV_PROP)))
  {
    u64 inv_weight = 0;
    for (unsigned i = 0; i < L; ++i)
      if (flags[i] & MST_FLAG_ONE) inv_weight += weights ? weights[i] : 1u;
    stats->inv_prop = (double)inv_weight / (double)sum_weights;
    ok = index_list(L, [&](size_t i) { return (flags[i] & MST_FLAG_ONE) != 0; }, &stats->inv_cols, &stats->inv_cols_count);
  }
  if (!ok) { pllhip_msa_destroy_stats(stats); return nullptr; }
  return stats;
}

PLL_EXPORT void pllhip_msa_stats_last_times(double * upload_ms, double * kernel_ms)
{
  if (upload_ms) *upload_ms = g_last_ms[0];
  if (kernel_ms) *kernel_ms = g_last_ms[1];
}

}
