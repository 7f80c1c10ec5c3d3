// The iterate ranges of the device-resident Newton-Raphson loop (pll-modules_amd/csrc/newton_range.hpp) on the CPU.
// A loop with the limit max_newton publishes base + 1 ... base + max_newton + 2 (modulo 2^32) in one word of its control
// block, one value per scan, and its workgroups wait for exactly those values.  The property: none of them is a value
// the word can hold when the loop starts.  The model here is brute force -- the set of all such values, kept value by
// value: 0 (the allocation, and the memset after a loop that was given up can come before any loop) and every value of
// the ranges of the HELD_LOOPS loops before (the previous loop may have ended at any scan; a loop whose launch failed
// published nothing and leaves what the loops before it left).
// Sequences of loops go through it with the rule of newton_range.hpp, from a counter at 0 and from counters just below
// 2^32; then the rule this one replaced -- the loop's sequence number times 256 -- goes through the same checker, which
// has to reject it with the loop after a loop of 257 scans.
// A program of its own, built with -fsanitize=address,undefined (tests/test_newton_range.py).  Prints "ok".
#include "newton_range.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <functional>
#include <unordered_map>
#include <vector>

constexpr unsigned HELD_LOOPS = 3;

struct Collision
{
  bool hit = false;
  unsigned loop = 0, scans = 0;          // the loop that waits for `value` after `scans` scans of its own ...
  uint32_t value = 0;
  int held_loop = -1;                    // ... which that loop published after `held_scans` scans (-1: the 0 of a memset)
  unsigned held_scans = 0, held_max_newton = 0;
};

// runs the loops `limits` (their max_newton) with bases from `rule`; the first collision, if any
static Collision check(const std::vector<unsigned> & limits, const std::function<uint32_t(unsigned)> & rule)
{
  struct Range { unsigned loop, max_newton; uint32_t base; };
  struct From { int loop; unsigned scans, max_newton; };
  std::deque<Range> before;
  std::unordered_map<uint32_t, From> held;                       // value -> who leaves it
  held[0u] = {-1, 0u, 0u};
  for (unsigned n = 0; n < limits.size(); ++n)
  {
    const unsigned m = limits[n];
    const uint32_t base = rule(m);
    for (uint64_t k = 1; k <= (uint64_t)m + 2; ++k)
    {
      const uint32_t v = (uint32_t)(base + k);
      const auto it = held.find(v);
      if (it == held.end()) continue;
      Collision c;
      c.hit = true; c.loop = n; c.scans = (unsigned)k; c.value = v;
      c.held_loop = it->second.loop; c.held_scans = it->second.scans; c.held_max_newton = it->second.max_newton;
      return c;
    }
    for (uint64_t k = 1; k <= (uint64_t)m + 2; ++k) held[(uint32_t)(base + k)] = {(int)n, (unsigned)k, m};
    before.push_back({n, m, base});
    if (before.size() > HELD_LOOPS)
    {
      const Range r = before.front();
      before.pop_front();
      for (uint64_t k = 1; k <= (uint64_t)r.max_newton + 2; ++k)
      {
        const auto it = held.find((uint32_t)(r.base + k));
        if (it != held.end() && it->second.loop == (int)r.loop) held.erase(it);
      }
    }
  }
  return Collision();
}

static void describe(const char * what, const Collision & c)
{
  if (c.held_loop < 0)
    printf("%s: loop %u waits for %u after %u scans: the value a memset leaves\n", what, c.loop, c.value, c.scans);
  else
    printf("%s: loop %u waits for %u after %u scans: loop %d (max_newton %u) leaves it after %u scans\n", what, c.loop,
           c.value, c.scans, c.held_loop, c.held_max_newton, c.held_scans);
}

static void require(bool ok, const char * what) { if (!ok) { printf("failed: %s\n", what); exit(1); } }

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint64_t splitmix64()
{
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

// mostly the limits callers use, now and then anything up to the bound
static std::vector<unsigned> random_limits(unsigned count)
{
  std::vector<unsigned> v(count);
  for (unsigned & m : v)
    m = 1u + (unsigned)(splitmix64() % ((splitmix64() & 15u) ? 600u : newton_range::MAX_NEWTON));
  return v;
}

int main()
{
  using newton_range::MAX_NEWTON;
  require(!newton_range::supported(0) && newton_range::supported(1) && newton_range::supported(MAX_NEWTON) &&
          !newton_range::supported(MAX_NEWTON + 1) && !newton_range::supported(~0u), "supported(): 1 ... MAX_NEWTON");
  require(MAX_NEWTON >= (1u << 16), "the bound is at least 2^16");
  require(newton_range::length(MAX_NEWTON) == MAX_NEWTON + 2 && newton_range::length(1) == 3, "length(): max_newton + 2");

  // every ordered pair of the fixed limits, as loops that follow one another
  const unsigned fixed[] = {1, 30, 254, 255, 256, 300, MAX_NEWTON};
  std::vector<unsigned> pairs;
  for (unsigned a : fixed) for (unsigned b : fixed) { pairs.push_back(a); pairs.push_back(b); }

  // counters at 0 and just below 2^32: the loop that would pass 2^32 - 1 is each of the first loops in turn
  // (all pairs and a long random sequence from a few of them, each fixed limit once and a short random sequence from all)
  const uint32_t below[] = {0u, 258u, MAX_NEWTON + 2, 1u, 2u, 3u, 4u, 31u, 32u, 33u, 256u, 257u, 259u, 302u, 303u, 1000u,
                            MAX_NEWTON, MAX_NEWTON + 1, MAX_NEWTON + 3, 2 * MAX_NEWTON + 4, 2 * MAX_NEWTON + 5};
  std::vector<uint32_t> starts(1, 0u);
  for (uint32_t d : below) starts.push_back(UINT32_MAX - d);
  for (size_t s = 0; s < starts.size(); ++s)
  {
    const uint32_t start = starts[s];
    bool wrap = false;
    for (int kind = 0; kind < 2; ++kind)
    {
      std::vector<unsigned> limits;
      if (kind) limits = random_limits(s == 0 ? 1500 : s < 4 ? 300 : 100);
      else if (s < 4) limits = pairs;
      else for (size_t k = 0; k < 7; ++k) limits.push_back(fixed[(k + s) % 7]);
      newton_range::Counter c;
      c.last = start;
      uint32_t seen = start;
      const Collision got = check(limits, [&](unsigned m) {
        const uint32_t base = newton_range::take(c, m);
        if (c.last < seen) wrap = true;
        seen = c.last;
        return base;
      });
      if (got.hit) { describe("newton_range::take", got); printf("counter started at %u\n", start); return 1; }
    }
    require(wrap == (s > 0), "the counters that start below 2^32 pass it, the one that starts at 0 does not");
  }

  // the rule before: loop number s (1, 2, ...) counted from s * 256 -- 256 values per loop, whatever max_newton
  auto old_rule = [](uint64_t & seq) { return [&seq](unsigned) { return (uint32_t)(++seq * 256u); }; };
  {
    uint64_t seq = 0;
    const Collision got = check({255, 32}, old_rule(seq));       // 257 scans at the most, then an ordinary loop
    require(got.hit, "the checker rejects sequence number * 256 for a loop after one of max_newton 255");
    describe("sequence number * 256", got);
    require(got.loop == 1 && got.scans == 1 && got.held_loop == 0 && got.held_scans == 257 && got.value == 513u,
            "... with the first wait of the loop after a loop of 257 scans");
  }
  {
    uint64_t seq = 0;
    const Collision got = check({300, 32}, old_rule(seq));       // a longer loop can end after 257 scans too
    require(got.hit && got.loop == 1 && got.scans == 1 && got.held_scans == 257, "... and after a longer loop");
  }
  {
    uint64_t seq = 0;
    require(!check({254, 32, 254, 254, 1, 30}, old_rule(seq)).hit, "256 scans per loop fitted sequence number * 256");
  }
  {
    uint64_t seq = 0;
    require(check(pairs, old_rule(seq)).hit, "the checker rejects sequence number * 256 on the pairs of limits");
  }
  printf("ok\n");
  return 0;
}
