// sim_plan.cpp -- see sim_plan.hpp
#include "sim_plan.hpp"

#include <algorithm>
#include <cstdio>

namespace simplan {

namespace {

bool fail(std::string & error, const char * fmt, unsigned a = 0, unsigned b = 0, unsigned c = 0)
{
  char buf[160];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  error = buf;
  return false;
}

struct Frame { unsigned node, slot, next; };

} // namespace

unsigned slot_bound(unsigned nodes)
{
  unsigned lg = 0;                                // ceil(log2(nodes))
  while (lg < 32 && (1ULL << lg) < nodes) ++lg;
  return lg > 2 ? lg - 1 : 1;
}

bool build(const Input & in, Plan & plan, std::string & error)
{
  plan = Plan();
  if (in.edge_count && (!in.parent || !in.child || !in.matrix)) return fail(error, "an edge array is missing");
  if (in.node_count < in.tips || !in.node_count)
    return fail(error, "node count %u is less than the %u tips", in.node_count, in.tips);
  if (in.root >= in.node_count) return fail(error, "root node %u out of range (%u nodes)", in.root, in.node_count);
  if (in.root < in.tips) return fail(error, "root node %u is a tip: a tip cannot be a parent", in.root);

  const unsigned n = in.node_count;
  std::vector<unsigned> parent_edge(n, NONE), nchildren(n, 0);
  std::vector<char> named(n, 0);
  named[in.root] = 1;
  for (unsigned k = 0; k < in.edge_count; ++k)
  {
    const unsigned p = in.parent[k], c = in.child[k];
    if (p >= n) return fail(error, "edge %u: node %u out of range (%u nodes)", k, p, n);
    if (c >= n) return fail(error, "edge %u: node %u out of range (%u nodes)", k, c, n);
    if (in.matrix[k] >= in.matrix_count)
      return fail(error, "edge %u: matrix index %u out of range (%u matrices)", k, in.matrix[k], in.matrix_count);
    if (p < in.tips) return fail(error, "edge %u: tip %u used as a parent", k, p);
    if (c == in.root || parent_edge[c] != NONE) return fail(error, "edge %u: node %u is reached twice", k, c);
    parent_edge[c] = k;
    nchildren[p]++;
    named[p] = named[c] = 1;
  }

  // children of every node, in edge order
  std::vector<unsigned> first(n + 1, 0), kids(in.edge_count);
  for (unsigned v = 0; v < n; ++v) first[v + 1] = first[v] + nchildren[v];
  {
    std::vector<unsigned> fill(first.begin(), first.end() - 1);
    for (unsigned k = 0; k < in.edge_count; ++k) kids[fill[in.parent[k]]++] = k;
  }

  // who the root reaches, parents before children
  std::vector<unsigned> order;
  order.reserve(n);
  plan.reached.assign(n, 0);
  order.push_back(in.root);
  plan.reached[in.root] = 1;
  for (size_t q = 0; q < order.size(); ++q)
    for (unsigned i = first[order[q]]; i < first[order[q] + 1]; ++i)
    {
      const unsigned c = in.child[kids[i]];
      plan.reached[c] = 1;                        // (once: every node has one parent edge)
      order.push_back(c);
    }
  for (unsigned v = 0; v < n; ++v)
    if (named[v] && !plan.reached[v]) return fail(error, "node %u is never reached from root node %u", v, in.root);
  for (unsigned t = 0; t < in.tips; ++t)
    if (!plan.reached[t]) return fail(error, "tip %u is missing from the edge list", t);
  plan.nodes_reached = (unsigned)order.size();
  plan.bound = slot_bound(plan.nodes_reached);

  // subtree sizes, then the children of every node lightest first (ties: by matrix index, so that the order of
  // the list does not show in the plan)
  std::vector<unsigned> size(n, 1);
  for (size_t q = order.size(); q-- > 1; ) size[in.parent[parent_edge[order[q]]]] += size[order[q]];
  for (unsigned v : order)
    std::sort(kids.begin() + first[v], kids.begin() + first[v + 1], [&](unsigned a, unsigned b) {
      const unsigned sa = size[in.child[a]], sb = size[in.child[b]];
      if (sa != sb) return sa < sb;
      if (in.matrix[a] != in.matrix[b]) return in.matrix[a] < in.matrix[b];
      return in.child[a] < in.child[b];
    });

  std::vector<unsigned> free_slots;               // kept descending: the smallest free slot is taken
  unsigned next_slot = 0, live = 0;
  auto take = [&]() {
    unsigned s;
    if (free_slots.empty()) s = next_slot++;
    else { s = free_slots.back(); free_slots.pop_back(); }
    plan.slots = std::max(plan.slots, ++live);
    return s;
  };
  auto give = [&](unsigned s) {
    free_slots.insert(std::upper_bound(free_slots.begin(), free_slots.end(), s, [](unsigned a, unsigned b) { return a > b; }), s);
    --live;
  };

  plan.steps.reserve(in.edge_count);
  std::vector<Frame> stack;
  stack.push_back({in.root, take(), first[in.root]});
  if (first[in.root] == first[in.root + 1]) give(stack.back().slot);
  while (!stack.empty())
  {
    Frame & f = stack.back();
    if (f.next == first[f.node + 1]) { stack.pop_back(); continue; }
    const unsigned k = kids[f.next++];
    const bool last = f.next == first[f.node + 1];
    const unsigned c = in.child[k];
    const bool leaf = first[c] == first[c + 1];   // nothing is drawn from it: it needs no slot
    Step s;
    s.parent = f.node;
    s.child = c;
    s.matrix = in.matrix[k];
    s.src = f.slot;
    s.dst = leaf ? NONE : last ? f.slot : take();
    plan.steps.push_back(s);
    if (last && leaf) give(f.slot);
    if (!leaf) stack.push_back({c, s.dst, first[c]});     // (invalidates f)
  }
  if (live != 0 || plan.slots > plan.bound)
    return fail(error, "internal: %u slots live at the end, %u used, bound %u", live, plan.slots, plan.bound);

  for (const Step & s : plan.steps) plan.matrices.push_back(s.matrix);
  std::sort(plan.matrices.begin(), plan.matrices.end());
  plan.matrices.erase(std::unique(plan.matrices.begin(), plan.matrices.end()), plan.matrices.end());
  return true;
}

} // namespace simplan
