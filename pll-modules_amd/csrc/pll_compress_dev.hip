// pll_compress_dev.hip -- pll_compress_site_patterns / pll_compress_site_patterns_msa on the device
// (kernels_compress.hpp; contract: INTEGRATION.md, "Alignment input"; design: DESIGN.md section 14).
//
// One call = one stream of its own on the device pllhip_get_device() names: rows up through a pinned staging buffer,
// hash, insert, prefix sum, gather, results down.  Everything the call allocates is gone when it returns.  The
// caller's rows and *length are written only after the last device operation has succeeded.
#include "device_job.hpp"
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

// the host copies, freed unless the call hands them on
struct HostResult
{
  uint8_t * rows = nullptr;                                   // the compressed rows
  unsigned * weights = nullptr;                               // the return value
  ~HostResult() { free(rows); free(weights); }
};

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
  int device = -1;
  if (!caller_device("pll_compress_site_patterns", &device)) return nullptr;

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

  HostResult host;
  DeviceJob j;
  MsaStager stager;
  if (!j.enter(device)) return nullptr;
  // start, uploaded, numbered (before the host reads the pattern count), gather queued, computed, downloaded
  hipEvent_t ev[6];
  for (hipEvent_t & e : ev) if (!(e = j.event())) return nullptr;
  uint8_t * d_in = j.alloc<uint8_t>((size_t)T * Lp, "the alignment");
  uint2 * d_hash = j.alloc<uint2>((size_t)L, "column hashes");            // after the insert: rank [L] and pat_site [L]
  unsigned long long * d_table = j.alloc<unsigned long long>(slots, "the pattern table");
  unsigned long long * d_scalars = j.alloc<unsigned long long>(4, "scalars");
  unsigned * d_owner = j.alloc<unsigned>((size_t)L, "group owners");
  unsigned * d_first = j.alloc<unsigned>((size_t)L, "first occurrences");
  unsigned * d_weight = j.alloc<unsigned>((size_t)L, "group sizes");
  unsigned * d_pat_weight = j.alloc<unsigned>((size_t)L, "pattern weights");
  unsigned * d_tiles = j.alloc<unsigned>((size_t)ntiles1 + ntiles2, "scan tiles");
  unsigned * d_site_pattern = site_pattern_map ? j.alloc<unsigned>((size_t)L, "the site -> pattern map") : nullptr;
  if (!d_in || !d_hash || !d_table || !d_scalars || !d_owner || !d_first || !d_weight || !d_pat_weight || !d_tiles ||
      (site_pattern_map && !d_site_pattern) || !stager.open(half))
    return nullptr;
  unsigned long long * h_scalars = j.pinned<unsigned long long>(4);      // {bad, total, probe steps, compares}
  if (!h_scalars) return nullptr;
  unsigned * d_rank = reinterpret_cast<unsigned *>(d_hash), * d_pat_site = d_rank + L;
  unsigned * d_tiles2 = d_tiles + ntiles1;
  unsigned * d_total = reinterpret_cast<unsigned *>(d_scalars + 1);

  // --- upload -----------------------------------------------------------------------------------------------------
  if (!hip_ok(hipEventRecord(ev[0], j.stream), "hipEventRecord") ||
      !stager.rows(j.stream, d_in, sequence, T, L, Lp, half) || !hip_ok(hipEventRecord(ev[1], j.stream), "hipEventRecord"))
    return nullptr;

  // --- groups, first occurrences, numbering -----------------------------------------------------------------------
  if (!hip_ok(hipMemsetAsync(d_table, 0xff, slots * sizeof(unsigned long long), j.stream), "memset table") ||
      !hip_ok(hipMemsetAsync(d_scalars, 0xff, sizeof(unsigned long long), j.stream), "memset scalars") ||
      !hip_ok(hipMemsetAsync(d_scalars + 1, 0, 3 * sizeof(unsigned long long), j.stream), "memset scalars") ||
      !hip_ok(hipMemsetAsync(d_first, 0xff, (size_t)L * sizeof(unsigned), j.stream), "memset first") ||
      !hip_ok(hipMemsetAsync(d_weight, 0, (size_t)L * sizeof(unsigned), j.stream), "memset weights"))
    return nullptr;
  hipLaunchKernelGGL(k_msa_hash, dim3(grid_for(((size_t)L + 3u) / 4u, MSA_WG)), dim3(MSA_WG), 0, j.stream,
                     (const uint8_t *)d_in, Lp, T, L, codes, hash_keep_mask("PLLHIP_COMPRESS_HASH_BITS"), slot_mask, d_hash,
                     d_scalars);
  hipLaunchKernelGGL(k_msa_insert, dim3(grid_for(L, MSA_WG)), dim3(MSA_WG), 0, j.stream, (const uint8_t *)d_in, Lp, T,
                     L, codes, (const uint2 *)d_hash, d_table, slot_mask, d_owner, d_first, d_weight,
                     d_scalars + 2);
  hipLaunchKernelGGL(k_msa_scan_tiles<true>, dim3(ntiles1), dim3(1024), 0, j.stream, (const unsigned *)nullptr,
                     (const unsigned *)d_owner, (const unsigned *)d_first, L, d_tiles);
  if (ntiles1 <= 1024u)
    hipLaunchKernelGGL(k_msa_scan_top, dim3(1), dim3(1024), 0, j.stream, d_tiles, ntiles1, d_total);
  else
  {
    hipLaunchKernelGGL(k_msa_scan_tiles<false>, dim3(ntiles2), dim3(1024), 0, j.stream, (const unsigned *)d_tiles,
                       (const unsigned *)nullptr, (const unsigned *)nullptr, ntiles1, d_tiles2);
    hipLaunchKernelGGL(k_msa_scan_top, dim3(1), dim3(1024), 0, j.stream, d_tiles2, ntiles2, d_total);
    hipLaunchKernelGGL(k_msa_scan_apply<false>, dim3(ntiles2), dim3(1024), 0, j.stream, d_tiles,
                       (const unsigned *)nullptr, (const unsigned *)nullptr, (const unsigned *)nullptr, ntiles1,
                       (const unsigned *)d_tiles2, (unsigned *)nullptr, (unsigned *)nullptr, (unsigned *)nullptr);
  }
  hipLaunchKernelGGL(k_msa_scan_apply<true>, dim3(ntiles1), dim3(1024), 0, j.stream, (unsigned *)nullptr,
                     (const unsigned *)d_owner, (const unsigned *)d_first, (const unsigned *)d_weight, L,
                     (const unsigned *)d_tiles, d_rank, d_pat_site, d_pat_weight);
  if (!hip_ok(hipGetLastError(), "compression kernels") || !hip_ok(hipEventRecord(ev[2], j.stream), "hipEventRecord") ||
      !hip_ok(hipMemcpyAsync(h_scalars, d_scalars, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, j.stream),
              "read pattern count") ||
      !hip_ok(hipStreamSynchronize(j.stream), "compression kernels"))
    return nullptr;
  if (h_scalars[0] != MSA_NO_BAD)
  {
    const unsigned long long t = h_scalars[0] / L, s = h_scalars[0] % L;
    const unsigned char c = (unsigned char)sequence[t][s];
    if (c >= 32 && c < 127)
      set_error(PLL_ERROR_TIPDATA_ILLEGALSTATE, "Illegal state code '%c' in sequence %llu, site %llu", c, t, s);
    else
      set_error(PLL_ERROR_TIPDATA_ILLEGALSTATE, "Illegal state code 0x%02x in sequence %llu, site %llu", (unsigned)c, t, s);
    return nullptr;
  }
  const unsigned P = (unsigned)h_scalars[1];
  if (P < 1u || P > L)
  {
    set_error(PLL_ERROR_HIP_RUNTIME, "pll_compress_site_patterns: %u patterns counted for %u sites", P, L);
    return nullptr;
  }

  // --- the compressed rows ----------------------------------------------------------------------------------------
  const size_t Pp = ((size_t)P + 3u) & ~(size_t)3u;
  uint8_t * d_out = j.alloc<uint8_t>((size_t)T * Pp, "the compressed alignment");
  if (!d_out) return nullptr;
  host.rows = (uint8_t *)malloc((size_t)T * Pp);
  host.weights = (unsigned *)malloc((size_t)P * sizeof(unsigned));
  if (!host.rows || !host.weights)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate %zu bytes for the compressed alignment", (size_t)T * Pp);
    return nullptr;
  }
  if (!hip_ok(hipEventRecord(ev[3], j.stream), "hipEventRecord")) return nullptr;
  hipLaunchKernelGGL(k_msa_gather, dim3(grid_for(Pp / 4u, MSA_WG), std::min(T, 1024u)), dim3(MSA_WG), 0, j.stream,
                     (const uint8_t *)d_in, Lp, T, P, Pp, (const unsigned *)d_pat_site, d_out);
  if (site_pattern_map)
    hipLaunchKernelGGL(k_msa_number, dim3(grid_for(L, MSA_WG)), dim3(MSA_WG), 0, j.stream, (const unsigned *)d_owner,
                       (const unsigned *)d_first, (const unsigned *)d_rank, L, d_site_pattern);
  if (!hip_ok(hipGetLastError(), "gather kernels") || !hip_ok(hipEventRecord(ev[4], j.stream), "hipEventRecord"))
    return nullptr;

  // --- download ---------------------------------------------------------------------------------------------------
  if (!hip_ok(hipMemcpyAsync(host.rows, d_out, (size_t)T * Pp, hipMemcpyDeviceToHost, j.stream), "download rows") ||
      !hip_ok(hipMemcpyAsync(host.weights, d_pat_weight, (size_t)P * sizeof(unsigned), hipMemcpyDeviceToHost, j.stream),
              "download weights") ||
      (site_pattern_map &&
       !hip_ok(hipMemcpyAsync(site_pattern_map, d_site_pattern, (size_t)L * sizeof(unsigned), hipMemcpyDeviceToHost,
                              j.stream), "download the site -> pattern map")) ||
      !hip_ok(hipEventRecord(ev[5], j.stream), "hipEventRecord") ||
      !hip_ok(hipStreamSynchronize(j.stream), "download"))
    return nullptr;
  // device segments only: the host's read of the pattern count and its allocations between ev[2] and ev[3] are not
  // kernel time
  float seg[5];
  for (int k = 0; k < 5; ++k)
    if (!j.elapsed(ev[k], ev[k + 1], &seg[k])) return nullptr;
  g_last_ms[0] = seg[0];
  g_last_ms[1] = (double)seg[1] + (double)seg[3];
  g_last_ms[2] = seg[4];
  g_last_counts[0] = h_scalars[2];
  g_last_counts[1] = h_scalars[3];

  // nothing can fail from here on: commit
  for (unsigned t = 0; t < T; ++t)
  {
    memcpy(sequence[t], host.rows + (size_t)t * Pp, P);
    sequence[t][P] = 0;
  }
  *length = (int)P;
  unsigned * result = host.weights;
  host.weights = nullptr;
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
