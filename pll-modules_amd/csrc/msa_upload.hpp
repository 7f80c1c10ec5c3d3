// msa_upload.hpp -- the rows of an alignment on the host -> one device array [T][Lp], through the two halves of a
// pinned staging buffer (shared by pll_compress_dev.hip and pll_msa_stats_dev.hip).
//
// Job provides: stream, d_in (uint8_t *, T * Lp bytes), h_stage (uint8_t *, pinned, 2 * half bytes) and
// half_free[2] (events: the copy out of a half has finished).
#pragma once

#include "engine.h"

#include <algorithm>
#include <cstring>

namespace pllhip {

template <typename Job>
bool upload_rows(Job & j, char ** sequence, unsigned T, unsigned L, size_t Lp, size_t half)
{
  unsigned turn = 0;
  bool used[2] = {false, false};
  auto send = [&](size_t dst_off, size_t bytes, unsigned h) {
    return hip_ok(hipMemcpyAsync(j.d_in + dst_off, j.h_stage + h * half, bytes, hipMemcpyHostToDevice, j.stream),
                  "upload alignment") &&
           hip_ok(hipEventRecord(j.half_free[h], j.stream), "hipEventRecord");
  };
  auto claim = [&](unsigned h) {
    if (used[h] && !hip_ok(hipEventSynchronize(j.half_free[h]), "hipEventSynchronize")) return false;
    used[h] = true;
    return true;
  };
  if (Lp <= half)
  {
    const unsigned per = (unsigned)std::min<size_t>(T, half / Lp);       // whole rows per half, at the device's stride
    for (unsigned t0 = 0; t0 < T; t0 += per, ++turn)
    {
      const unsigned h = turn & 1u, n = std::min(per, T - t0);
      if (!claim(h)) return false;
      for (unsigned r = 0; r < n; ++r) memcpy(j.h_stage + h * half + (size_t)r * Lp, sequence[t0 + r], L);
      if (!send((size_t)t0 * Lp, (size_t)(n - 1u) * Lp + L, h)) return false;
    }
  }
  else
    for (unsigned t = 0; t < T; ++t)
      for (size_t off = 0; off < L; off += half, ++turn)
      {
        const unsigned h = turn & 1u;
        const size_t n = std::min(half, (size_t)L - off);
        if (!claim(h)) return false;
        memcpy(j.h_stage + h * half, sequence[t] + off, n);
        if (!send((size_t)t * Lp + off, n, h)) return false;
      }
  return true;
}

} // namespace pllhip
