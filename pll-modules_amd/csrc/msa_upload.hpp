// msa_upload.hpp -- the rows of an alignment on the host -> one device array [T][Lp], through the two halves of a
// pinned staging buffer (pll_compress_dev.hip, pll_msa_stats_dev.hip, pll_distance_dev.hip).
#pragma once

#include "device_job.hpp"

#include <algorithm>
#include <cstring>

namespace pllhip {

// the staging buffer (2 * half bytes) and, per half, the event "the copy out of it has finished"
struct MsaStager
{
  PinnedBuf<uint8_t> stage;
  hipEvent_t half_free[2] = {nullptr, nullptr};
  bool used[2] = {false, false};

  // (a copy out of the buffer may still be queued where a call has failed)
  ~MsaStager()
  {
    for (int h = 0; h < 2; ++h)
    {
      if (used[h]) (void)hipEventSynchronize(half_free[h]);
      if (half_free[h]) (void)hipEventDestroy(half_free[h]);
    }
  }

  bool open(size_t half)
  {
    for (hipEvent_t & e : half_free)
      if (!hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate")) return false;
    return stage.alloc(2u * half);
  }

  // d_in: T * Lp bytes
  bool rows(hipStream_t stream, uint8_t * d_in, char ** sequence, unsigned T, unsigned L, size_t Lp, size_t half)
  {
    unsigned turn = 0;
    uint8_t * const h_stage = stage.p;
    auto send = [&](size_t dst_off, size_t bytes, unsigned h) {
      return hip_ok(hipMemcpyAsync(d_in + dst_off, h_stage + h * half, bytes, hipMemcpyHostToDevice, stream),
                    "upload alignment") &&
             hip_ok(hipEventRecord(half_free[h], stream), "hipEventRecord");
    };
    auto claim = [&](unsigned h) {
      if (used[h] && !hip_ok(hipEventSynchronize(half_free[h]), "hipEventSynchronize")) return false;
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
        for (unsigned r = 0; r < n; ++r) memcpy(h_stage + h * half + (size_t)r * Lp, sequence[t0 + r], L);
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
          memcpy(h_stage + h * half, sequence[t] + off, n);
          if (!send((size_t)t * Lp + off, n, h)) return false;
        }
    return true;
  }
};

} // namespace pllhip
