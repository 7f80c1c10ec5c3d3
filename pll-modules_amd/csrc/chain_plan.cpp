// The chain planner (chain_plan.hpp).
#include "chain_plan.hpp"
#include <algorithm>
#include <utility>

namespace chainplan {

bool analyse_list(const ChainList & list, ListFacts & facts)
{
  const unsigned count = list.count;
  std::vector<int> made_by(list.nodes, -1), sc_writer(list.nscalers, -1);
  std::vector<char> read_ext(list.nodes, 0), sc_read_ext(list.nscalers, 0);
  facts.producer.assign(2 * (size_t)count, -1);
  facts.consumer.assign(count, -1);
  facts.readers.assign(count, 0); facts.size.assign(count, 1);
  facts.heavy.assign(count, 0); facts.plain.assign(count, 0);
  for (unsigned k = 0; k < count; ++k)
  {
    const pll_operation_t & op = list.ops[k];
    const unsigned child[2] = {op.child1_clv_index, op.child2_clv_index};
    const int child_sc[2] = {op.child1_scaler_index, op.child2_scaler_index};
    if (child[0] == child[1] || op.parent_clv_index == child[0] || op.parent_clv_index == child[1]) return false;
    int * pr = &facts.producer[2 * (size_t)k];
    for (int c = 0; c < 2; ++c)
    {
      pr[c] = made_by[child[c]];
      if (child[c] < list.coded_below && child_sc[c] == PLL_SCALE_BUFFER_NONE) facts.plain[k] |= (unsigned char)(1 << c);
      if (pr[c] < 0)
      {
        read_ext[child[c]] = 1;
        if (child_sc[c] >= 0)
        {
          if (sc_writer[child_sc[c]] >= 0) return false;
          sc_read_ext[child_sc[c]] = 1;
        }
      }
      else
      {
        if (++facts.readers[pr[c]] > 1) return false;
        if (child_sc[c] != list.ops[pr[c]].parent_scaler_index) return false;
        facts.consumer[pr[c]] = (int)k;
      }
    }
    if (made_by[op.parent_clv_index] >= 0 || read_ext[op.parent_clv_index]) return false;
    made_by[op.parent_clv_index] = (int)k;
    if (op.parent_scaler_index >= 0)
    {
      if (sc_writer[op.parent_scaler_index] >= 0 || sc_read_ext[op.parent_scaler_index]) return false;
      sc_writer[op.parent_scaler_index] = (int)k;
    }
    facts.size[k] = 1 + (pr[0] >= 0 ? facts.size[pr[0]] : 0) + (pr[1] >= 0 ? facts.size[pr[1]] : 0);
    // the heavy child: the one with the larger subtree, child 1 on a tie
    if (pr[0] >= 0 && (pr[1] < 0 || facts.size[pr[0]] >= facts.size[pr[1]])) facts.heavy[k] = 1;
    else if (pr[1] >= 0) facts.heavy[k] = 2;
  }
  return true;
}

// Chains: an operation continues the chain of its heavy child while the chain has room (max_len operations, lds_cap
// doubles of tables), else it starts one; a chain runs in the round after the chains whose vectors it reads from memory.
void plan_chains(const ChainList & list, const ListFacts & facts, unsigned max_len, unsigned lds_cap, ChainPlan & plan)
{
  const unsigned count = list.count;
  std::vector<int> chain_of(count, -1);
  plan = ChainPlan();
  plan.carried.assign(count, 0);
  for (unsigned k = 0; k < count; ++k)
  {
    const int pr[2] = {facts.producer[2 * k], facts.producer[2 * k + 1]};
    const unsigned cost = list.lds(k);
    int heavy = (int)facts.heavy[k] - 1;          // which child (0 / 1) continues a chain
    if (heavy >= 0 && (plan.chains[chain_of[pr[heavy]]].size() >= max_len ||
                       plan.lds[chain_of[pr[heavy]]] + cost > lds_cap)) heavy = -1;
    int round = 0;
    for (int c = 0; c < 2; ++c)
      if (pr[c] >= 0 && c != heavy) round = std::max(round, plan.launch[chain_of[pr[c]]] + 1);
    if (heavy >= 0)
    {
      const int ch = chain_of[pr[heavy]];
      plan.chains[ch].push_back(k);
      plan.lds[ch] += cost;
      plan.launch[ch] = std::max(plan.launch[ch], round);
      plan.carried[k] = (unsigned char)(heavy + 1);
      chain_of[k] = ch;
    }
    else
    {
      chain_of[k] = (int)plan.chains.size();
      plan.chains.push_back(std::vector<unsigned>(1, k));
      plan.lds.push_back(cost);
      plan.launch.push_back(round);
    }
    plan.rounds = std::max(plan.rounds, plan.launch[chain_of[k]] + 1);
  }
}

// Folded cherries.  The vector that an operation reads next to the handed-over one comes back from memory -- unless it
// is a lone cherry (a tip x tip operation that is a chain of its own): that one the consumer can build in registers
// from the two tip tables, at the price of fold_lds doubles of the chain's LDS.  LDS is what ends chains, and a cut
// costs a read as well (the handed-over vector comes back from memory), so cuts and folds are chosen together: per
// heavy path (the operations linked by their heavy child, which is what plan_chains' chains are pieces of) a dynamic
// programme picks the cut points that minimise
//     vectors read from memory = cuts + foldable cherries that are not folded
// under the caps (max_len operations per chain, not counting the folded ones; lds_cap doubles including the folds'
// tables); within a piece as many cherries are folded as fit.  Ties go to fewer cuts.  Without a foldable cherry, or
// when the optimum folds nothing, `plan` stays what plan_chains made it -- whose greedy cuts are the fewest possible --,
// so the result never reads more than the plan without folds.
// `plan`: plan_chains' result for the same arguments.
void plan_folds(const ChainList & list, const ListFacts & facts, unsigned max_len, unsigned lds_cap, unsigned fold_lds,
                ChainPlan & plan)
{
  const unsigned count = list.count;
  if (!fold_lds || count < 2) return;
  std::vector<int> up(count, -1), cherry(count, -1);    // the next operation of the path; the foldable light child
  bool any = false;
  for (unsigned k = 0; k < count; ++k)
  {
    if (!facts.heavy[k]) continue;
    up[facts.heavy_producer(k)] = (int)k;
    const int light = facts.light_producer(k);
    if (light >= 0 && facts.cherry((unsigned)light)) { cherry[k] = light; any = true; }
  }
  if (!any) return;

  // per path: the pieces [a, b] and how many cherries each folds
  struct Piece { unsigned a, b, folds; };
  std::vector<std::vector<unsigned>> paths;
  std::vector<std::vector<Piece>> pieces;
  unsigned nfolds = 0;
  for (unsigned k = 0; k < count; ++k)
  {
    if (facts.heavy[k]) continue;                 // not the bottom of a path
    std::vector<unsigned> path;
    for (int x = (int)k; x >= 0; x = up[x]) path.push_back((unsigned)x);
    const unsigned n = (unsigned)path.size();
    // best[i]: the first i operations of the path; value = (pieces - folds, pieces), smallest first
    const long INF = 1L << 40;
    std::vector<long> best(n + 1, INF);
    std::vector<unsigned> from(n + 1, 0), nf(n + 1, 0);
    best[0] = 0;
    for (unsigned b = 0; b < n; ++b)
    {
      unsigned lds = 0, foldable = 0;
      for (unsigned a = b + 1; a-- > 0 && b - a < max_len; )
      {
        lds += list.lds(path[a]);
        if (lds > lds_cap) break;
        if (cherry[path[a]] >= 0) ++foldable;
        if (best[a] >= INF) continue;
        const unsigned folds = std::min(foldable, (lds_cap - lds) / fold_lds);
        const long v = best[a] + (1L - (long)folds) * 4096L + 1L;
        if (v < best[b + 1]) { best[b + 1] = v; from[b + 1] = a; nf[b + 1] = folds; }
      }
    }
    if (best[n] >= INF) return;                   // (an operation whose own tables exceed the cap: plan_chains' plan stands)
    std::vector<Piece> pc;
    for (unsigned i = n; i > 0; i = from[i]) pc.push_back({from[i], i - 1, nf[i]});
    std::reverse(pc.begin(), pc.end());
    for (const Piece & x : pc) nfolds += x.folds;
    paths.push_back(std::move(path));
    pieces.push_back(std::move(pc));
  }
  if (!nfolds) return;

  // the chains: the pieces of the paths, numbered by their first operation as plan_chains numbers them; a folded
  // cherry (a path of one operation) goes in front of its consumer instead of forming a chain
  std::vector<char> is_folded(count, 0);
  std::vector<std::pair<unsigned, std::vector<unsigned>>> made;     // (first operation, chain)
  std::vector<unsigned> made_lds;
  ChainPlan out;
  out.carried.assign(count, 0);
  out.folded.assign(count, 0);
  for (size_t p = 0; p < paths.size(); ++p)
    for (const Piece & x : pieces[p])
    {
      unsigned left = x.folds;
      for (unsigned j = x.a; j <= x.b && left; ++j)
        if (cherry[paths[p][j]] >= 0) { is_folded[cherry[paths[p][j]]] = 1; --left; }
    }
  for (size_t p = 0; p < paths.size(); ++p)
  {
    if (paths[p].size() == 1 && is_folded[paths[p][0]]) continue;
    for (const Piece & x : pieces[p])
    {
      std::vector<unsigned> ch;
      unsigned lds = 0;
      for (unsigned j = x.a; j <= x.b; ++j)
      {
        const unsigned k = paths[p][j];
        if (cherry[k] >= 0 && is_folded[cherry[k]])
        {
          ch.push_back((unsigned)cherry[k]);
          out.folded[cherry[k]] = (unsigned char)(3 - facts.heavy[k]);      // the child that is not the heavy one
          lds += fold_lds;
        }
        ch.push_back(k);
        lds += list.lds(k);
        out.carried[k] = j > x.a ? facts.heavy[k] : 0;
      }
      made.emplace_back(paths[p][x.a], std::move(ch));
      made_lds.push_back(lds);
    }
  }
  std::vector<size_t> idx(made.size());
  for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return made[a].first < made[b].first; });
  std::vector<int> chain_of(count, -1);
  for (size_t i : idx)
  {
    for (unsigned k : made[i].second) chain_of[k] = (int)out.chains.size();
    out.chains.push_back(std::move(made[i].second));
    out.lds.push_back(made_lds[i]);
  }
  // rounds: a chain runs after the chains whose last vector it reads from memory (a folded cherry is no chain)
  out.launch.assign(out.chains.size(), 0);
  for (unsigned k = 0; k < count; ++k)
  {
    for (int c = 0; c < 2; ++c)
    {
      const int pk = facts.producer[2 * k + c];
      if (pk >= 0 && chain_of[pk] != chain_of[k])
        out.launch[chain_of[k]] = std::max(out.launch[chain_of[k]], out.launch[chain_of[pk]] + 1);
    }
    out.rounds = std::max(out.rounds, out.launch[chain_of[k]] + 1);
  }
  plan = std::move(out);
}

// Children read through class tables.  The vector of a cherry depends on the pair of tip codes of a site alone, the one
// of a cherry x tip operation on three codes: at most U^2 / U^3 different columns for U codes in use (lut_used), however
// long the alignment.  Where a chain meets such a child as its light child -- the vector that comes back from memory
// next to the handed-over one --, the consumer gathers rows of P . vector(class) from a table of all classes instead
// (built per traversal by the class kernels of site repeats; the class code is arithmetic on the tip codes).
// Nothing else changes: the child's own chain runs and stores vector and counts as before, no chain, cut or fold moves.
// Marked: an operation's inner child that is neither handed over nor folded, made by an operation of the list that is
// a cherry of coded tips or such a cherry x a coded tip, with at most max_classes classes; one child per operation
// (it becomes child 2, as a folded cherry does), none next to a fold.
void plan_lookups(const ListFacts & facts, unsigned lut_used, unsigned max_classes, ChainPlan & plan)
{
  const unsigned count = facts.count();
  plan.lookups.clear();
  plan.looked.clear();
  if (!max_classes || count < 2) return;
  std::vector<char> fold_consumer(count, 0);
  if (!plan.folded.empty())
    for (const std::vector<unsigned> & ch : plan.chains)
      for (size_t i = 0; i + 1 < ch.size(); ++i)
        if (plan.folded[ch[i]]) fold_consumer[ch[i + 1]] = 1;
  const unsigned long long u = lut_used;
  for (unsigned k = 0; k < count; ++k)
    for (unsigned x = 0; x < 2 && !fold_consumer[k]; ++x)
    {
      const int top = facts.producer[2 * k + x];
      if (top < 0 || plan.carried[k] == x + 1 || (!plan.folded.empty() && plan.folded[top])) continue;
      int cherry = -1;
      unsigned long long classes = u * u;
      if (!facts.cherry((unsigned)top))
      {
        const unsigned tips = facts.plain[top];
        if (tips != 1 && tips != 2) continue;
        cherry = facts.producer[2 * top + (tips == 1 ? 1 : 0)];
        if (cherry < 0 || !facts.cherry((unsigned)cherry)) continue;
        classes *= u;
      }
      if (classes > max_classes) continue;
      if (plan.looked.empty()) plan.looked.assign(count, 0);
      plan.looked[k] = (unsigned char)(x + 1);
      plan.lookups.push_back({k, (unsigned)top, cherry, (unsigned)classes});
      break;
    }
}

// Deferred stores.  Folds and class tables took the READS of small tip-only subtrees out of the traversal; their
// vectors were still written, 8 * S * R bytes per site each, although no operation of the list reads them from memory:
//   a folded cherry             -- its consumer builds the block in registers;
//   a looked-up child           -- its consumer gathers rows of the class table; the child's own chain (the cherry, or
//                                  the cherry handed over in registers to the cherry x tip operation) feeds nobody else.
// Such an operation is marked "parent vector not stored" (PlanOp::flags bit 0).  Coded tips and P-matrices alone
// recompute it, so the engine keeps it as its operation (unstored.hpp, as for an evaluate-only traversal) and stores it
// for the first reader or before an input changes.  Scaler counts are written as always.  The cherry below a looked-up
// cherry x tip is marked only where that operation takes it over in registers.  Level 2: the looked-up children keep
// their stores.
// Levels 3 and 4 are one walk up every chain with one test: the next operation of the chain that is not a folded cherry
// takes this vector in registers, and it is the vector's only reader in the list.  So never the last operation of a
// chain, never a vector that an operation reads from memory or that nobody in the list reads.
//   a vector inside a chain (level 4) -- every operation that passes the test, whatever its children are, however far
//     up the chain.  The next evaluation overwrites it unread.  Such a vector is recomputed from stored child vectors,
//     not from tip codes alone: the engine stores it before one of them is overwritten (UnstoredLedger::before_list).
//   a tip-only run at the bottom of a chain (level 3) -- the same walk, as far as the result depends on tip codes
//     alone: from the chain's first operation that is not folded, which has to be a cherry of coded tips, over the
//     operations "handed-over child x coded tip", the first `depth` of them at the most (0: all), up to the first that
//     fails the test or hands its vector across a folded cherry.
// plan.run_up links two marked operations that stand next to each other in a chain (UnstoredLedger::recompute_list
// stores a run in one list); across a folded cherry there is no link, and the reader of the lower one stores what it needs alone.
// `plan`: after plan_folds and plan_lookups.
void plan_defers(const ListFacts & facts, DeferPolicy policy, ChainPlan & plan)
{
  const unsigned count = facts.count(), level = policy.level;
  plan.deferred.clear();
  plan.run_up.clear();
  const bool folds_only = level == 2;
  if ((level < 3 || count < 2) && plan.folded.empty() && (folds_only || plan.lookups.empty())) return;
  plan.deferred.assign(count, 0);
  for (unsigned k = 0; k < count && !plan.folded.empty(); ++k)
    if (plan.folded[k]) plan.deferred[k] = 1;
  if (folds_only) return;
  for (const ChainPlan::Lookup & l : plan.lookups)
  {
    plan.deferred[l.top] = 1;
    if (l.cherry < 0) continue;
    const unsigned side = facts.producer[2 * l.top] == l.cherry ? 1u : 2u;
    if (plan.carried[l.top] == side) plan.deferred[l.cherry] = 1;
  }
  if (level < 3 || count < 2) return;
  const bool runs_only = level == 3;
  auto is_folded = [&](unsigned k) { return !plan.folded.empty() && plan.folded[k]; };
  // operation `o` takes the vector of operation `from` in registers
  auto taken_over = [&](unsigned o, unsigned from)
  { return plan.carried[o] && facts.producer[2 * o + plan.carried[o] - 1] == (int)from; };
  for (const std::vector<unsigned> & ch : plan.chains)
  {
    size_t below = ch.size();                          // position of the operation marked last
    unsigned len = 0;                                  // marked operations
    for (size_t i = 0; i + 1 < ch.size(); ++i)
    {
      const unsigned k = ch[i];
      if (is_folded(k)) continue;
      // (level 3: a cherry, then handed-over child x coded tip -- the child of k that is not the handed-over one)
      const bool tip_only = len ? ((facts.plain[k] >> (2 - plan.carried[k])) & 1) != 0 : facts.cherry(k);
      if (runs_only && (!tip_only || (policy.depth && len >= policy.depth))) break;
      const size_t next = i + 1 + (is_folded(ch[i + 1]) ? 1 : 0);
      if (next >= ch.size() || !taken_over(ch[next], k) || facts.readers[k] != 1)
      {
        if (runs_only) break;
        continue;
      }
      plan.deferred[k] = 1;
      if (below + 1 == i)
      {
        if (plan.run_up.empty()) plan.run_up.assign(count, -1);
        plan.run_up[ch[below]] = (int)k;
      }
      below = i;
      ++len;
      if (runs_only && next != i + 1) break;
    }
  }
}

// Order of the chains.  By rounds: round by round, longest chains first within a round (their workgroups are
// dispatched first).  Otherwise depth first, so that a vector is consumed soon after it was written (the kernel
// walks slabs of sites through ALL chains: what a slab wrote a few chains ago is still in L2 / the memory-side
// cache).  The chains form a tree -- chain c feeds the chain that reads c's last vector as a child from memory --
// and the larger feeder goes first, which keeps the number of results waiting for their consumer small.
std::vector<size_t> chain_order(const ListFacts & facts, const ChainPlan & plan, bool by_rounds)
{
  const size_t nch = plan.chains.size();
  std::vector<size_t> order;
  order.reserve(nch);
  if (by_rounds)
  {
    for (size_t c = 0; c < nch; ++c) order.push_back(c);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b)
    {
      if (plan.launch[a] != plan.launch[b]) return plan.launch[a] < plan.launch[b];
      return plan.chains[a].size() > plan.chains[b].size();
    });
    return order;
  }
  std::vector<int> chain_at(facts.count(), -1);
  std::vector<unsigned> weight(nch, 0);
  std::vector<std::vector<size_t>> feeders(nch);
  std::vector<char> is_feeder(nch, 0);
  for (size_t c = 0; c < nch; ++c)
    for (unsigned k : plan.chains[c]) chain_at[k] = (int)c;
  for (size_t c = 0; c < nch; ++c)                  // chains are numbered in creation order: feeders first
  {
    weight[c] += (unsigned)plan.chains[c].size();
    for (unsigned k : plan.chains[c])
      for (int x = 0; x < 2; ++x)
      {
        const int pk = facts.producer[2 * k + x];
        if (pk < 0 || chain_at[pk] == (int)c) continue;
        feeders[c].push_back((size_t)chain_at[pk]);
        is_feeder[chain_at[pk]] = 1;
        weight[c] += weight[chain_at[pk]];
      }
  }
  std::vector<std::pair<size_t, size_t>> stack;   // (chain, next feeder)
  for (size_t root = 0; root < nch; ++root)
  {
    if (is_feeder[root]) continue;
    stack.emplace_back(root, 0);
    while (!stack.empty())
    {
      const size_t c = stack.back().first;
      if (stack.back().second == 0)
        std::stable_sort(feeders[c].begin(), feeders[c].end(), [&](size_t a, size_t b) { return weight[a] > weight[b]; });
      if (stack.back().second < feeders[c].size()) { const size_t f = feeders[c][stack.back().second++]; stack.emplace_back(f, 0); }
      else { order.push_back(c); stack.pop_back(); }
    }
  }
  return order;
}

} // namespace chainplan
