// sim_plan_host_check.cpp -- the simulation planner (pll-modules_amd/csrc/sim_plan.cpp) on the CPU, as a program of
// its own (tests/test_simulate_reference.py builds it with -fsanitize=address,undefined and runs it).
//
// Ladder, balanced and random trees of 3, 4, 33 and 500 tips and a star, each as given and with its edge list
// reversed: the program is replayed with a liveness bookkeeping of its own -- every node has a state before it is
// read, no slot is shared by two live nodes, every tip is drawn once -- and the slot maximum is held against the
// derived bound.  Then every malformed list is rejected with its message.
#include "sim_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace simplan;

namespace {

int failures = 0;

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++failures; } } while (0)

unsigned long long mix(unsigned long long seed, unsigned long long c)
{
  unsigned long long z = seed + (c + 1ULL) * 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

struct EdgeList
{
  unsigned tips = 0, nodes = 0, root = 0, matrices = 0;       // matrices 0: as many as edges
  std::vector<unsigned> parent, child, matrix;
  Input input() const
  {
    Input in;
    in.tips = tips;
    in.node_count = nodes;
    in.matrix_count = matrices ? matrices : (unsigned)matrix.size();
    in.root = root;
    in.edge_count = (unsigned)parent.size();
    in.parent = parent.data();
    in.child = child.data();
    in.matrix = matrix.data();
    return in;
  }
};

// an unrooted binary tree grown by splitting edges (kind 0: the edge added last, a caterpillar; 1: the pendant edges
// in turn, balanced; 2: a random edge), directed away from inner node `tips`
EdgeList grow(unsigned tips, int kind, unsigned long long seed)
{
  std::vector<std::pair<unsigned, unsigned>> edges = {{0, tips}, {1, tips}, {2, tips}};
  for (unsigned t = 3; t < tips; ++t)
  {
    size_t e = edges.size() - 1;
    if (kind == 2) e = (size_t)(mix(seed, t) % edges.size());
    if (kind == 1)
    {
      // the shallowest pendant edge: breadth-first growth keeps the tree balanced
      std::vector<unsigned> depth(2 * tips, 0);
      std::vector<std::vector<unsigned>> adj(2 * tips);
      for (auto & ed : edges) { adj[ed.first].push_back(ed.second); adj[ed.second].push_back(ed.first); }
      std::vector<unsigned> queue = {tips};
      std::vector<char> seen(2 * tips, 0);
      seen[tips] = 1;
      for (size_t q = 0; q < queue.size(); ++q)
        for (unsigned w : adj[queue[q]])
          if (!seen[w]) { seen[w] = 1; depth[w] = depth[queue[q]] + 1; queue.push_back(w); }
      unsigned best = ~0u;
      for (size_t k = 0; k < edges.size(); ++k)
      {
        const unsigned tip = edges[k].first < tips ? edges[k].first : edges[k].second;
        if (tip < tips && depth[tip] < best) { best = depth[tip]; e = k; }
      }
    }
    const unsigned u = edges[e].first, v = edges[e].second, w = tips + (t - 2);
    edges[e] = {u, w};
    edges.push_back({w, v});
    edges.push_back({t, w});
  }
  EdgeList L;
  L.tips = tips;
  L.nodes = 2 * tips - 2;
  L.root = tips;
  std::vector<std::vector<std::pair<unsigned, unsigned>>> adj(L.nodes);
  for (unsigned k = 0; k < edges.size(); ++k)
  {
    adj[edges[k].first].push_back({edges[k].second, k});
    adj[edges[k].second].push_back({edges[k].first, k});
  }
  std::vector<std::pair<unsigned, unsigned>> stack = {{L.root, NONE}};
  while (!stack.empty())
  {
    const auto [v, from] = stack.back();
    stack.pop_back();
    for (auto [w, k] : adj[v])
      if (w != from)
      {
        L.parent.push_back(v);
        L.child.push_back(w);
        L.matrix.push_back(k);
        stack.push_back({w, v});
      }
  }
  return L;
}

EdgeList star(unsigned tips)
{
  EdgeList L;
  L.tips = tips;
  L.nodes = tips + 1;
  L.root = tips;
  for (unsigned t = 0; t < tips; ++t) { L.parent.push_back(tips); L.child.push_back(t); L.matrix.push_back(t); }
  return L;
}

void replay(const EdgeList & L, const char * name)
{
  Plan plan;
  std::string error;
  const Input in = L.input();
  if (!build(in, plan, error)) { CHECK(false, "%s: rejected: %s", name, error.c_str()); return; }
  CHECK(plan.steps.size() == L.parent.size(), "%s: %zu steps for %zu edges", name, plan.steps.size(), L.parent.size());
  CHECK(plan.nodes_reached == L.nodes, "%s: %u nodes reached", name, plan.nodes_reached);
  CHECK(plan.bound == slot_bound(plan.nodes_reached), "%s: bound", name);
  CHECK(plan.slots >= 1 && plan.slots <= plan.bound, "%s: %u slots, bound %u", name, plan.slots, plan.bound);

  std::vector<unsigned> remaining(L.nodes, 0);
  for (unsigned p : L.parent) remaining[p]++;
  std::vector<char> has_state(L.nodes, 0);
  std::vector<unsigned> owner(plan.slots, NONE);                // the live node in each slot
  has_state[L.root] = 1;
  owner[0] = L.root;
  unsigned live = 1, live_max = 1;
  for (const Step & s : plan.steps)
  {
    CHECK(s.parent < L.nodes && s.child < L.nodes, "%s: node out of range", name);
    CHECK(has_state[s.parent], "%s: node %u is read before it has a state", name, s.parent);
    CHECK(!has_state[s.child], "%s: node %u is drawn twice", name, s.child);
    CHECK(s.src < plan.slots && owner[s.src] == s.parent, "%s: slot %u does not hold node %u", name, s.src, s.parent);
    CHECK(remaining[s.parent] > 0, "%s: node %u has no child left", name, s.parent);
    has_state[s.child] = 1;
    const bool parent_dies = --remaining[s.parent] == 0;
    if (parent_dies) { owner[s.src] = NONE; --live; }
    if (s.dst != NONE)
    {
      CHECK(s.dst < plan.slots, "%s: slot %u out of range", name, s.dst);
      CHECK(remaining[s.child] > 0, "%s: node %u keeps a slot without children", name, s.child);
      CHECK(owner[s.dst] == NONE, "%s: slot %u is given to node %u while node %u lives in it", name, s.dst, s.child,
            owner[s.dst]);
      owner[s.dst] = s.child;
      ++live;
    }
    else
      CHECK(remaining[s.child] == 0, "%s: node %u has children and no slot", name, s.child);
    live_max = std::max(live_max, live);
  }
  CHECK(live == 0, "%s: %u nodes live at the end", name, live);
  CHECK(live_max == plan.slots, "%s: %u slots live at most, the plan says %u", name, live_max, plan.slots);
  for (unsigned v = 0; v < L.nodes; ++v) CHECK(has_state[v], "%s: node %u never gets a state", name, v);

  // the steps are the edges of the list
  std::vector<unsigned long long> a, b;
  for (size_t k = 0; k < L.parent.size(); ++k)
    a.push_back(((unsigned long long)L.parent[k] << 42) | ((unsigned long long)L.child[k] << 21) | L.matrix[k]);
  for (const Step & s : plan.steps) b.push_back(((unsigned long long)s.parent << 42) | ((unsigned long long)s.child << 21) | s.matrix);
  std::sort(a.begin(), a.end());
  std::sort(b.begin(), b.end());
  CHECK(a == b, "%s: the steps are not the edges", name);
  CHECK(std::is_sorted(plan.matrices.begin(), plan.matrices.end()) && plan.matrices.size() == L.matrix.size(),
        "%s: matrix list", name);
  printf("%-22s nodes %4u  slots %u  bound %u\n", name, plan.nodes_reached, plan.slots, plan.bound);
}

void both_orders(EdgeList L, const std::string & name)
{
  replay(L, name.c_str());
  Plan first, second;
  std::string error;
  const bool ok1 = build(L.input(), first, error);
  std::reverse(L.parent.begin(), L.parent.end());
  std::reverse(L.child.begin(), L.child.end());
  std::reverse(L.matrix.begin(), L.matrix.end());
  replay(L, (name + " reversed").c_str());
  const bool ok2 = build(L.input(), second, error);
  bool same = ok1 && ok2 && first.steps.size() == second.steps.size();
  for (size_t k = 0; same && k < first.steps.size(); ++k)
    same = memcmp(&first.steps[k], &second.steps[k], sizeof(Step)) == 0;
  CHECK(same, "%s: the plan depends on the order of the list", name.c_str());
}

void rejected(const EdgeList & L, const char * what, const char * message)
{
  Plan plan;
  std::string error;
  const bool ok = build(L.input(), plan, error);
  CHECK(!ok, "%s: accepted", what);
  CHECK(ok || error == message, "%s: message \"%s\", expected \"%s\"", what, error.c_str(), message);
}

void malformed()
{
  const EdgeList good = grow(5, 2, 7);
  {
    EdgeList L = good;                                          // a node reached twice
    L.parent.push_back(L.root);
    L.child.push_back(L.child[3]);
    L.matrix.push_back(0);
    char msg[96];
    snprintf(msg, sizeof(msg), "edge %zu: node %u is reached twice", L.parent.size() - 1, L.child[3]);
    rejected(L, "reached twice", msg);
  }
  {
    EdgeList L = good;                                          // an edge back into the root
    L.parent.push_back(6);
    L.child.push_back(L.root);
    L.matrix.push_back(0);
    char msg[96];
    snprintf(msg, sizeof(msg), "edge %zu: node %u is reached twice", L.parent.size() - 1, L.root);
    rejected(L, "root reached", msg);
  }
  {
    EdgeList L = good;                                          // a tip as a parent
    L.nodes += 1;
    L.parent.push_back(2);
    L.child.push_back(L.nodes - 1);
    L.matrix.push_back(0);
    char msg[96];
    snprintf(msg, sizeof(msg), "edge %zu: tip 2 used as a parent", L.parent.size() - 1);
    rejected(L, "tip parent", msg);
  }
  {
    EdgeList L = good;                                          // a pair of nodes apart from the tree
    L.nodes += 2;
    L.parent.push_back(L.nodes - 2);
    L.child.push_back(L.nodes - 1);
    L.matrix.push_back(0);
    char msg[96];
    snprintf(msg, sizeof(msg), "node %u is never reached from root node %u", L.nodes - 2, L.root);
    rejected(L, "never reached", msg);
  }
  {
    EdgeList L = good;                                          // a cycle apart from the tree
    L.nodes += 2;
    L.parent.push_back(L.nodes - 2); L.child.push_back(L.nodes - 1); L.matrix.push_back(0);
    L.parent.push_back(L.nodes - 1); L.child.push_back(L.nodes - 2); L.matrix.push_back(1);
    char msg[96];
    snprintf(msg, sizeof(msg), "node %u is never reached from root node %u", L.nodes - 2, L.root);
    rejected(L, "cycle", msg);
  }
  {
    EdgeList L = good;                                          // a tip missing
    L.matrices = (unsigned)L.matrix.size();
    size_t k = 0;
    while (L.child[k] != 1) ++k;
    L.parent.erase(L.parent.begin() + k);
    L.child.erase(L.child.begin() + k);
    L.matrix.erase(L.matrix.begin() + k);
    rejected(L, "tip missing", "tip 1 is missing from the edge list");
  }
  {
    EdgeList L = good;
    L.child[2] = L.nodes;
    char msg[96];
    snprintf(msg, sizeof(msg), "edge 2: node %u out of range (%u nodes)", L.nodes, L.nodes);
    rejected(L, "node range", msg);
  }
  {
    EdgeList L = good;
    Input in = L.input();
    in.matrix_count = 3;
    size_t k = 0;
    while (L.matrix[k] < 3) ++k;
    Plan plan;
    std::string error;
    char msg[96];
    snprintf(msg, sizeof(msg), "edge %zu: matrix index %u out of range (3 matrices)", k, L.matrix[k]);
    CHECK(!build(in, plan, error) && error == msg, "matrix range: \"%s\"", error.c_str());
  }
  {
    EdgeList L = good;
    L.root = 1;
    rejected(L, "root tip", "root node 1 is a tip: a tip cannot be a parent");
    L.root = L.nodes + 3;
    char msg[96];
    snprintf(msg, sizeof(msg), "root node %u out of range (%u nodes)", L.root, L.nodes);
    rejected(L, "root range", msg);
  }
}

} // namespace

int main()
{
  const unsigned sizes[] = {3, 4, 33, 500};
  const char * kinds[] = {"ladder", "balanced", "random"};
  for (unsigned tips : sizes)
    for (int kind = 0; kind < 3; ++kind)
      both_orders(grow(tips, kind, 1000 + tips), std::string(kinds[kind]) + " " + std::to_string(tips));
  both_orders(star(3), "star 3");
  both_orders(star(40), "star 40");
  {
    // the caterpillar needs one slot, whatever its length
    Plan plan;
    std::string error;
    const EdgeList L = grow(500, 0, 0);
    CHECK(build(L.input(), plan, error) && plan.slots == 1, "ladder 500: %u slots", plan.slots);
  }
  malformed();
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
