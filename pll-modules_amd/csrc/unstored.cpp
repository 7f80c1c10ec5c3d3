// The ledger of unstored vectors (unstored.hpp).
#include "unstored.hpp"

namespace unstored {

void UnstoredLedger::reset(unsigned nodes, unsigned nmat)
{
  count_ = 0;
  live_.assign(nodes, 0);
  op_.assign(nodes, pll_operation_t());
  run_up_.assign(nodes, -1);
  mat_users_.assign(nmat, 0);
  row_ = 0;
  row_mark_ = 0;
}

void UnstoredLedger::drop(unsigned node, bool dead)
{
  if (!count_ || !live_[node]) return;
  const pll_operation_t & o = op_[node];
  const bool deferred = live_[node] == TRANSIENT_DEFERRED;
  live_[node] = 0;
  --mat_users_[o.child1_matrix_index];
  --mat_users_[o.child2_matrix_index];
  --count_;
  if (dead && deferred) stats_deferred_.given_up++;
  else if (dead) stats_mode_.discarded++;
}

void UnstoredLedger::mark(const pll_operation_t & o, char kind)
{
  drop(o.parent_clv_index, true);
  live_[o.parent_clv_index] = kind;
  op_[o.parent_clv_index] = o;
  run_up_[o.parent_clv_index] = -1;
  ++mat_users_[o.child1_matrix_index];
  ++mat_users_[o.child2_matrix_index];
  ++count_;
  if (kind == TRANSIENT_DEFERRED) stats_deferred_.deferred++;
  else stats_mode_.skipped++;
}

void UnstoredLedger::before_list(const pll_operation_t * ops, unsigned count, unsigned nscalers, bool busy,
                                 std::vector<unsigned> & want, std::vector<char> & going) const
{
  want.clear();
  going.clear();
  if (!count_ || busy) return;
  going.assign(live_.size(), 0);
  std::vector<char> swritten(nscalers, 0);
  for (unsigned k = 0; k < count; ++k)
  {
    const unsigned child[2] = {ops[k].child1_clv_index, ops[k].child2_clv_index};
    for (int x = 0; x < 2; ++x)
      if (live_[child[x]] && !going[child[x]]) want.push_back(child[x]);
    going[ops[k].parent_clv_index] = 1;
    if (ops[k].parent_scaler_index >= 0) swritten[ops[k].parent_scaler_index] = 1;
  }
  for (unsigned t = 0; t < live_.size(); ++t)
  {
    if (!live_[t] || going[t]) continue;
    const pll_operation_t & o = op_[t];
    if (going[o.child1_clv_index] || going[o.child2_clv_index] ||
        (o.child1_scaler_index >= 0 && swritten[o.child1_scaler_index]) ||
        (o.child2_scaler_index >= 0 && swritten[o.child2_scaler_index]) ||
        (o.parent_scaler_index >= 0 && swritten[o.parent_scaler_index]))
      want.push_back(t);
  }
}

void UnstoredLedger::recompute_list(const std::vector<unsigned> & want, bool group, const std::vector<char> * going,
                                    std::vector<pll_operation_t> & out_ops, unsigned & out_ndeferred) const
{
  out_ops.clear();
  out_ndeferred = 0;
  if (!count_) return;
  const unsigned nodes = (unsigned)live_.size();
  std::vector<char> seen(nodes, 0);
  std::vector<std::pair<unsigned, unsigned>> stack;   // (node, children looked at)
  for (unsigned w : want)
  {
    if (group && w < nodes && live_[w] == TRANSIENT_DEFERRED)
      for (unsigned steps = 0; steps < nodes; ++steps)      // up the run, while its links hold (unstored.hpp, 3.)
      {
        const int up = run_up_[w];
        if (up < 0 || live_[up] != TRANSIENT_DEFERRED || (going && (*going)[up])) break;
        const pll_operation_t & o = op_[up];
        if (o.child1_clv_index != w && o.child2_clv_index != w) break;
        w = (unsigned)up;
      }
    if (w >= nodes || !live_[w] || seen[w]) continue;
    seen[w] = 1;
    stack.emplace_back(w, 0u);
    while (!stack.empty())
    {
      const unsigned node = stack.back().first;
      const pll_operation_t & o = op_[node];
      if (stack.back().second < 2)
      {
        const unsigned c = stack.back().second++ ? o.child2_clv_index : o.child1_clv_index;
        if (live_[c] && !seen[c]) { seen[c] = 1; stack.emplace_back(c, 0u); }
      }
      else
      {
        if (live_[node] == TRANSIENT_DEFERRED) ++out_ndeferred;
        out_ops.push_back(o);
        stack.pop_back();
      }
    }
  }
}

void UnstoredLedger::after_list(const pll_operation_t * ops, unsigned count, const std::vector<unsigned> & left_out_parents,
                                const std::vector<std::pair<unsigned, unsigned>> & runs, char kind)
{
  if (!left_out_parents.empty())
  {
    std::vector<int> by_parent(live_.size(), -1);
    for (unsigned k = 0; k < count; ++k) by_parent[ops[k].parent_clv_index] = (int)k;
    for (unsigned parent : left_out_parents)
      if (by_parent[parent] >= 0) mark(ops[by_parent[parent]], kind);
  }
  if (kind == TRANSIENT_DEFERRED)
    for (const std::pair<unsigned, unsigned> & r : runs)
      if (live_[r.first] == TRANSIENT_DEFERRED && live_[r.second] == TRANSIENT_DEFERRED) run_up_[r.first] = (int)r.second;
}

void UnstoredLedger::discard_mode_vectors()
{
  for (unsigned n = 0; n < live_.size() && count_; ++n)
    if (live_[n] == TRANSIENT_MODE) drop(n, true);
}

} // namespace unstored
