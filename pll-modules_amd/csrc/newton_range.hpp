// The device-resident Newton-Raphson loop: which values of NewtonControl::iter a loop may use.  Host arithmetic on
// 32-bit integers alone: it knows nothing of the engine or of devices and builds with any C++ compiler
// (tests/newton_range_host_check.cpp runs it under ASan + UBSan against a brute-force model).
//
// The workgroups of a loop hand iterates to one another through one word of the control block: after scan `it`
// (0, 1, ...) the block that applies the step rule publishes base + it + 1, and the others wait for exactly that value
// (kernels_s20.hpp, newton_step_and_wait).  The host does not write the word between loops, so when a loop starts it
// holds whatever an earlier loop published last -- any value of that loop's range, for it may have ended at any scan --
// or 0: after the allocation, and after the memset that follows a loop that was given up (newton_finish).  A loop with
// the iteration limit max_newton makes at most max_newton + 2 scans (scan max_newton + 1 is the one that finds the limit
// exceeded), so its range is base + 1 ... base + max_newton + 2, modulo 2^32.
//
// The rule: a running counter per control block holds the highest value handed out so far; a loop's base is that value,
// and the counter advances by the loop's own max_newton + 2.  Ranges of successive loops therefore never share a value,
// whatever their lengths.  Where base + max_newton + 2 would pass 2^32 - 1 the loop starts again from base 0: its range
// 1 ... max_newton + 2 leaves 0 out, and lies below the range before it because max_newton is bounded (MAX_NEWTON: two
// ranges together are far shorter than 2^32).
#pragma once
#include <cstdint>

namespace newton_range {

// the largest max_newton the device loop takes (pllhip_newton_branch answers PLLHIP_ERROR_NEWTON_UNSUPPORTED above it)
constexpr uint32_t MAX_NEWTON = 1u << 16;

struct Counter { uint32_t last = 0; };          // the highest value handed out (0: none yet)

inline bool supported(unsigned max_newton) { return max_newton >= 1 && max_newton <= MAX_NEWTON; }

// values a loop with this limit may publish
inline uint32_t length(unsigned max_newton) { return (uint32_t)max_newton + 2u; }

// the base of the next loop (NewtonParams::iter_base); supported(max_newton) holds
inline uint32_t take(Counter & c, unsigned max_newton)
{
  const uint32_t len = length(max_newton);
  uint32_t base = c.last;
  if (base > UINT32_MAX - len) base = 0;        // the range would pass 2^32 - 1: from the bottom again, 0 left out
  c.last = base + len;
  return base;
}

} // namespace newton_range
