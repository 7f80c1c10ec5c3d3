// pll_compress_dev.hip -- pll_compress_site_patterns / pll_compress_site_patterns_msa on the device
// (kernels_compress.hpp; contract: INTEGRATION.md, "Alignment input"; design: DESIGN.md section 14).
//
// One call = one stream of its own on the device pllhip_get_device() names: rows up through a pinned staging buffer,
// hash, insert, prefix sum, gather, results down.  Everything the call allocates is gone when it returns.  The
// caller's rows and *length are written only after the last device operation has succeeded.
#include "engine.h"
#include "kernels_compress.hpp"
#include "msa_upload.hpp"
#include "pllhip.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

using namespace pllhip;

namespace {

constexpr size_t MSA_STAGE_BYTES = (size_t)16 << 20;          // one half of the staging buffer

thread_local double g_last_ms[3] = {0.0, 0.0, 0.0};           // upload, kernels, download of the last call
thread_local unsigned long long g_last_counts[2] = {0, 0};    // probe steps, full column compares of the last call

// everything a call owns on the device and in pinned memory
struct CompressJob
{
  int saved_device = -1;
  hipStream_t stream = nullptr;
  // start, uploaded, numbered (before the host reads the pattern count), gather queued, computed, downloaded
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipEvent_t half_free[2] = {nullptr, nullptr};
  uint8_t * h_stage = nullptr;
  unsigned long long * h_scalars = nullptr;                   // pinned: {bad, total, probe steps, compares}
  uint8_t * d_in = nullptr, * d_out = nullptr;
  uint2 * d_hash = nullptr;                                   // after the insert: rank [L] and pat_site [L]
  unsigned long long * d_table = nullptr, * d_scalars = nullptr;
  unsigned * d_owner = nullptr, * d_first = nullptr, * d_weight = nullptr, * d_pat_weight = nullptr;
  unsigned * d_tiles = nullptr, * d_site_pattern = nullptr;
  uint8_t * rows = nullptr;                                   // host copy of the compressed rows
  unsigned * weights = nullptr;                               // the return value

  ~CompressJob()
  {
    if (stream) (void)hipStreamSynchronize(stream);
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_hash); (void)hipFree(d_table); (void)hipFree(d_scalars);
    (void)hipFree(d_owner); (void)hipFree(d_first); (void)hipFree(d_weight); (void)hipFree(d_pat_weight);
    (void)hipFree(d_tiles); (void)hipFree(d_site_pattern);
    if (h_stage) (void)hipHostFree(h_stage);
    if (h_scalars) (void)hipHostFree(h_scalars);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : half_free) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    free(rows);
    free(weights);
    if (saved_device >= 0) (void)hipSetDevice(saved_device);
  }
};

template <typename T>
bool job_alloc(T ** ptr, size_t count, const char * what)
{
  *ptr = nullptr;
  const hipError_t err = hipMalloc(reinterpret_cast<void **>(ptr), (count ? count : 1) * sizeof(T));
  if (err == hipSuccess) return true;
  *ptr = nullptr;
  (void)hipGetLastError();
  set_error(PLL_ERROR_MEM_ALLOC, "hipMalloc of %zu bytes for %s failed: %s", (count ? count : 1) * sizeof(T), what,
            hipGetErrorString(err));
  return false;
}

unsigned grid_for(size_t items, unsigned per_block)
{
  return (unsigned)std::max<size_t>(1, std::min<size_t>((items + per_block - 1) / per_block, 4096));
}

// PLLHIP_COMPRESS_HASH_BITS=<0..64>: only that many bits of both hashes are used (a test knob: with few bits the
// full compare and the probing carry the result)
unsigned long long hash_keep_mask()
{
  const char * env = getenv("PLLHIP_COMPRESS_HASH_BITS");
  if (!env || !*env) return ~0ULL;
  const long bits = std::max(0L, std::min(64L, atol(env)));
  return bits >= 64 ? ~0ULL : ((1ULL << bits) - 1ULL);
}

unsigned * compress(char ** sequence, const pll_state_t * map, int count, int * length, unsigned * site_pattern_map)
{
  if (!sequence || !map || !length || count < 1 || *length < 1)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pll_compress_site_patterns: a NULL argument, or no sequence or no site");
    return nullptr;
  }
  for (int t = 0; t < count; ++t)
    if (!sequence[t])
    {
      set_error(PLL_ERROR_PARAM_INVALID, "pll_compress_site_patterns: sequence %d is NULL", t);
      return nullptr;
    }
  const int device = pllhip_get_device();
  if (device < 0 || device >= pllhip_device_count())
  {
    set_error(PLL_ERROR_HIP_NODEVICE, "pll_compress_site_patterns runs on HIP device %d; %d visible", device,
              pllhip_device_count());
    return nullptr;
  }

  // canonical codes: equal map value <=> equal code
  MsaCodes codes;
  {
    pll_state_t seen[256];
    unsigned nseen = 0;
    for (unsigned c = 0; c < 256; ++c)
    {
      if (!map[c]) { codes.code[c] = (uint16_t)MSA_ILLEGAL; continue; }
      unsigned k = 0;
      while (k < nseen && seen[k] != map[c]) ++k;
      if (k == nseen) seen[nseen++] = map[c];
      codes.code[c] = (uint16_t)k;
    }
  }

  const unsigned T = (unsigned)count, L = (unsigned)*length;
  const size_t Lp = ((size_t)L + 255u) & ~(size_t)255u;
  size_t slots = 2;
  while (slots < 2u * (size_t)L) slots <<= 1;                  // 2 * pow2ceil(L) <= 2^32
  const unsigned slot_mask = (unsigned)(slots - 1u);
  const unsigned ntiles1 = (unsigned)(((size_t)L + MSA_SCAN_TILE - 1u) / MSA_SCAN_TILE);
  const unsigned ntiles2 = (ntiles1 + MSA_SCAN_TILE - 1u) / MSA_SCAN_TILE;   // <= 128
  const size_t half = std::min(MSA_STAGE_BYTES, (size_t)T * Lp);

  CompressJob j;
  if (!hip_ok(hipGetDevice(&j.saved_device), "hipGetDevice") || !hip_ok(hipSetDevice(device), "hipSetDevice") ||
      !hip_ok(hipStreamCreateWithFlags(&j.stream, hipStreamNonBlocking), "hipStreamCreate"))
    return nullptr;
  for (hipEvent_t & e : j.ev) if (!hip_ok(hipEventCreate(&e), "hipEventCreate")) return nullptr;
  for (hipEvent_t & e : j.half_free)
    if (!hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate")) return nullptr;
  if (!job_alloc(&j.d_in, (size_t)T * Lp, "the alignment") || !job_alloc(&j.d_hash, (size_t)L, "column hashes") ||
      !job_alloc(&j.d_table, slots, "the pattern table") || !job_alloc(&j.d_scalars, 4, "scalars") ||
      !job_alloc(&j.d_owner, (size_t)L, "group owners") || !job_alloc(&j.d_first, (size_t)L, "first occurrences") ||
      !job_alloc(&j.d_weight, (size_t)L, "group sizes") || !job_alloc(&j.d_pat_weight, (size_t)L, "pattern weights") ||
      !job_alloc(&j.d_tiles, (size_t)ntiles1 + ntiles2, "scan tiles") ||
      (site_pattern_map && !job_alloc(&j.d_site_pattern, (size_t)L, "the site -> pattern map")))
    return nullptr;
  hipError_t herr = hipHostMalloc(reinterpret_cast<void **>(&j.h_stage), 2u * half);
  if (herr == hipSuccess) herr = hipHostMalloc(reinterpret_cast<void **>(&j.h_scalars), 4 * sizeof(unsigned long long));
  if (herr != hipSuccess)
  {
    (void)hipGetLastError();
    set_error(PLL_ERROR_MEM_ALLOC, "hipHostMalloc of the staging buffer (%zu bytes) failed: %s", 2u * half,
              hipGetErrorString(herr));
    return nullptr;
  }
  unsigned * d_rank = reinterpret_cast<unsigned *>(j.d_hash), * d_pat_site = d_rank + L;
  unsigned * d_tiles2 = j.d_tiles + ntiles1;
  unsigned * d_total = reinterpret_cast<unsigned *>(j.d_scalars + 1);

  // --- upload -----------------------------------------------------------------------------------------------------
  if (!hip_ok(hipEventRecord(j.ev[0], j.stream), "hipEventRecord") || !upload_rows(j, sequence, T, L, Lp, half) ||
      !hip_ok(hipEventRecord(j.ev[1], j.stream), "hipEventRecord"))
    return nullptr;

  // --- groups, first occurrences, numbering -----------------------------------------------------------------------
  if (!hip_ok(hipMemsetAsync(j.d_table, 0xff, slots * sizeof(unsigned long long), j.stream), "memset table") ||
      !hip_ok(hipMemsetAsync(j.d_scalars, 0xff, sizeof(unsigned long long), j.stream), "memset scalars") ||
      !hip_ok(hipMemsetAsync(j.d_scalars + 1, 0, 3 * sizeof(unsigned long long), j.stream), "memset scalars") ||
      !hip_ok(hipMemsetAsync(j.d_first, 0xff, (size_t)L * sizeof(unsigned), j.stream), "memset first") ||
      !hip_ok(hipMemsetAsync(j.d_weight, 0, (size_t)L * sizeof(unsigned), j.stream), "memset weights"))
    return nullptr;
  hipLaunchKernelGGL(k_msa_hash, dim3(grid_for(((size_t)L + 3u) / 4u, MSA_WG)), dim3(MSA_WG), 0, j.stream,
                     (const uint8_t *)j.d_in, Lp, T, L, codes, hash_keep_mask(), slot_mask, j.d_hash, j.d_scalars);
  hipLaunchKernelGGL(k_msa_insert, dim3(grid_for(L, MSA_WG)), dim3(MSA_WG), 0, j.stream, (const uint8_t *)j.d_in, Lp, T,
                     L, codes, (const uint2 *)j.d_hash, j.d_table, slot_mask, j.d_owner, j.d_first, j.d_weight,
                     j.d_scalars + 2);
  hipLaunchKernelGGL(k_msa_scan_tiles<true>, dim3(ntiles1), dim3(1024), 0, j.stream, (const unsigned *)nullptr,
                     (const unsigned *)j.d_owner, (const unsigned *)j.d_first, L, j.d_tiles);
  if (ntiles1 <= 1024u)
    hipLaunchKernelGGL(k_msa_scan_top, dim3(1), dim3(1024), 0, j.stream, j.d_tiles, ntiles1, d_total);
  else
  {
    hipLaunchKernelGGL(k_msa_scan_tiles<false>, dim3(ntiles2), dim3(1024), 0, j.stream, (const unsigned *)j.d_tiles,
                       (const unsigned *)nullptr, (const unsigned *)nullptr, ntiles1, d_tiles2);
    hipLaunchKernelGGL(k_msa_scan_top, dim3(1), dim3(1024), 0, j.stream, d_tiles2, ntiles2, d_total);
    hipLaunchKernelGGL(k_msa_scan_apply<false>, dim3(ntiles2), dim3(1024), 0, j.stream, j.d_tiles,
                       (const unsigned *)nullptr, (const unsigned *)nullptr, (const unsigned *)nullptr, ntiles1,
                       (const unsigned *)d_tiles2, (unsigned *)nullptr, (unsigned *)nullptr, (unsigned *)nullptr);
  }
  hipLaunchKernelGGL(k_msa_scan_apply<true>, dim3(ntiles1), dim3(1024), 0, j.stream, (unsigned *)nullptr,
                     (const unsigned *)j.d_owner, (const unsigned *)j.d_first, (const unsigned *)j.d_weight, L,
                     (const unsigned *)j.d_tiles, d_rank, d_pat_site, j.d_pat_weight);
  if (!hip_ok(hipGetLastError(), "compression kernels") || !hip_ok(hipEventRecord(j.ev[2], j.stream), "hipEventRecord") ||
      !hip_ok(hipMemcpyAsync(j.h_scalars, j.d_scalars, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, j.stream),
              "read pattern count") ||
      !hip_ok(hipStreamSynchronize(j.stream), "compression kernels"))
    return nullptr;
  if (j.h_scalars[0] != MSA_NO_BAD)
  {
    const unsigned long long t = j.h_scalars[0] / L, s = j.h_scalars[0] % L;
    const unsigned char c = (unsigned char)sequence[t][s];
    if (c >= 32 && c < 127)
      set_error(PLL_ERROR_TIPDATA_ILLEGALSTATE, "Illegal state code '%c' in sequence %llu, site %llu", c, t, s);
    else
      set_error(PLL_ERROR_TIPDATA_ILLEGALSTATE, "Illegal state code 0x%02x in sequence %llu, site %llu", (unsigned)c, t, s);
    return nullptr;
  }
  const unsigned P = (unsigned)j.h_scalars[1];
  if (P < 1u || P > L)
  {
    set_error(PLL_ERROR_HIP_RUNTIME, "pll_compress_site_patterns: %u patterns counted for %u sites", P, L);
    return nullptr;
  }

  // --- the compressed rows ----------------------------------------------------------------------------------------
  const size_t Pp = ((size_t)P + 3u) & ~(size_t)3u;
  if (!job_alloc(&j.d_out, (size_t)T * Pp, "the compressed alignment")) return nullptr;
  j.rows = (uint8_t *)malloc((size_t)T * Pp);
  j.weights = (unsigned *)malloc((size_t)P * sizeof(unsigned));
  if (!j.rows || !j.weights)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate %zu bytes for the compressed alignment", (size_t)T * Pp);
    return nullptr;
  }
  if (!hip_ok(hipEventRecord(j.ev[3], j.stream), "hipEventRecord")) return nullptr;
  hipLaunchKernelGGL(k_msa_gather, dim3(grid_for(Pp / 4u, MSA_WG), std::min(T, 1024u)), dim3(MSA_WG), 0, j.stream,
                     (const uint8_t *)j.d_in, Lp, T, P, Pp, (const unsigned *)d_pat_site, j.d_out);
  if (site_pattern_map)
    hipLaunchKernelGGL(k_msa_number, dim3(grid_for(L, MSA_WG)), dim3(MSA_WG), 0, j.stream, (const unsigned *)j.d_owner,
                       (const unsigned *)j.d_first, (const unsigned *)d_rank, L, j.d_site_pattern);
  if (!hip_ok(hipGetLastError(), "gather kernels") || !hip_ok(hipEventRecord(j.ev[4], j.stream), "hipEventRecord"))
    return nullptr;

  // --- download ---------------------------------------------------------------------------------------------------
  if (!hip_ok(hipMemcpyAsync(j.rows, j.d_out, (size_t)T * Pp, hipMemcpyDeviceToHost, j.stream), "download rows") ||
      !hip_ok(hipMemcpyAsync(j.weights, j.d_pat_weight, (size_t)P * sizeof(unsigned), hipMemcpyDeviceToHost, j.stream),
              "download weights") ||
      (site_pattern_map &&
       !hip_ok(hipMemcpyAsync(site_pattern_map, j.d_site_pattern, (size_t)L * sizeof(unsigned), hipMemcpyDeviceToHost,
                              j.stream), "download the site -> pattern map")) ||
      !hip_ok(hipEventRecord(j.ev[5], j.stream), "hipEventRecord") ||
      !hip_ok(hipStreamSynchronize(j.stream), "download"))
    return nullptr;
  // device segments only: the host's read of the pattern count and its allocations between ev[2] and ev[3] are not
  // kernel time
  float seg[5];
  for (int k = 0; k < 5; ++k)
    if (!hip_ok(hipEventElapsedTime(&seg[k], j.ev[k], j.ev[k + 1]), "hipEventElapsedTime")) return nullptr;
  g_last_ms[0] = seg[0];
  g_last_ms[1] = (double)seg[1] + (double)seg[3];
  g_last_ms[2] = seg[4];
  g_last_counts[0] = j.h_scalars[2];
  g_last_counts[1] = j.h_scalars[3];

  // nothing can fail from here on: commit
  for (unsigned t = 0; t < T; ++t)
  {
    memcpy(sequence[t], j.rows + (size_t)t * Pp, P);
    sequence[t][P] = 0;
  }
  *length = (int)P;
  unsigned * result = j.weights;
  j.weights = nullptr;
  return result;
}

} // namespace

extern "C" {

PLL_EXPORT unsigned int * pll_compress_site_patterns(char ** sequence, const pll_state_t * map, int count, int * length)
{
  return compress(sequence, map, count, length, nullptr);
}

PLL_EXPORT unsigned int * pll_compress_site_patterns_msa(pll_msa_t * msa, const pll_state_t * map,
                                                         unsigned int * site_pattern_map)
{
  if (!msa)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "pll_compress_site_patterns_msa: NULL alignment");
    return nullptr;
  }
  return compress(msa->sequence, map, msa->count, &msa->length, site_pattern_map);
}

PLL_EXPORT void pllhip_compress_last_counts(unsigned long long * probe_steps, unsigned long long * compares)
{
  if (probe_steps) *probe_steps = g_last_counts[0];
  if (compares) *compares = g_last_counts[1];
}

PLL_EXPORT void pllhip_compress_last_times(double * upload_ms, double * kernel_ms, double * download_ms)
{
  if (upload_ms) *upload_ms = g_last_ms[0];
  if (kernel_ms) *kernel_ms = g_last_ms[1];
  if (download_ms) *download_ms = g_last_ms[2];
}

}
