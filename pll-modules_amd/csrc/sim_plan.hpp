// sim_plan.hpp -- the host plan of a simulation along a tree (pll_simulate_dev.hip; contract: INTEGRATION.md,
// "Simulated alignments"; design: DESIGN.md section 28).  Host only: standard headers, no engine, no HIP, so that
// tests/sim_plan_host_check.cpp builds it on its own.
//
// The plan validates an edge list (parent -> child, matrix), orders it depth-first from the root and gives every inner
// node a slot that holds its states while its children are drawn.  A node's children are visited lightest subtree
// first; the heaviest child comes last and takes its parent's slot over (the draw reads the parent's state and writes
// the child's into the same place), a tip takes no slot at all -- its states go straight to the output.  So the slots
// alive at a node are its own and those of the ancestors that the path entered through a light edge.
//
// Bound.  size(v) = nodes in the subtree of v.  A light child c of v has a sibling at least as heavy, so
// 2 size(c) <= size(v) - 1.  An inner node x reached over k >= 1 light edges has 2 <= size(x) < n / 2^k
// (n = nodes reached), i.e. k + 1 < log2(n): the plan never uses more than slot_bound(n) = max(1, ceil(log2 n) - 1)
// slots, whatever the shape -- one on a caterpillar.  build() checks its own maximum against it.
#pragma once

#include <string>
#include <vector>

namespace simplan {

constexpr unsigned NONE = ~0u;

struct Input
{
  unsigned tips = 0;            // nodes below this index are tips
  unsigned node_count = 0;      // node indices are < node_count
  unsigned matrix_count = 0;    // matrix indices are < matrix_count
  unsigned root = 0;
  unsigned edge_count = 0;
  const unsigned * parent = nullptr, * child = nullptr, * matrix = nullptr;
};

// one draw: the child's state from the parent's, through the cumulated rows of `matrix`
struct Step
{
  unsigned parent, child;       // node indices
  unsigned matrix;
  unsigned src;                 // slot of the parent
  unsigned dst;                 // slot of the child (== src: it takes the parent's over; NONE: a tip)
};

struct Plan
{
  std::vector<Step> steps;              // depth-first from the root, whose slot is 0
  std::vector<unsigned> matrices;       // the distinct matrix indices of the steps, ascending
  std::vector<char> reached;            // [node_count]
  unsigned nodes_reached = 0;
  unsigned slots = 0;                   // slots in use at the same time, at most
  unsigned bound = 0;                   // slot_bound(nodes_reached)
};

unsigned slot_bound(unsigned nodes);

// false: `error` names the offender and `plan` is unspecified
bool build(const Input & in, Plan & plan, std::string & error);

} // namespace simplan
