// The ledger of unstored vectors (pll-modules_amd/csrc/unstored.hpp) on the CPU: hand-built lists on a partition of
// 4 tips (0 .. 3), up to 6 inner nodes (4 .. 9), 3 matrices and 3 scale buffers -- the smallest shapes at which each
// rule can go wrong --, with the expected values written out.  After every call that changes the ledger its fields
// are held against the invariants of unstored.hpp.
// A program of its own, built with -fsanitize=address,undefined (tests/test_unstored.py).  Prints "ok".
#include "unstored.hpp"
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

using namespace unstored;

constexpr unsigned NODES = 10, NMAT = 3, NSCALERS = 3;
constexpr char MODE = TRANSIENT_MODE, DEFERRED = TRANSIENT_DEFERRED;
typedef std::vector<unsigned> Nodes;
typedef std::vector<std::pair<unsigned, unsigned>> Runs;

static const char * section = "";
static void require_at(bool ok, const char * what, int line)
{
  if (!ok) { printf("failed (%s, line %d): %s\n", section, line, what); exit(1); }
}
#define require(cond) require_at((cond), #cond, __LINE__)

namespace unstored {
struct UnstoredLedgerCheck
{
  static int run_up(const UnstoredLedger & l, unsigned node) { return l.run_up_[node]; }
  // 1. the count is the number of live entries, 2. the user counts of the matrices are those of the live operations
  // (3., when a link holds, is what the cases of `runs` go through)
  static void invariants(const UnstoredLedger & l, int line)
  {
    unsigned live = 0;
    std::vector<unsigned> users(l.mat_users_.size(), 0);
    for (unsigned n = 0; n < l.live_.size(); ++n)
    {
      if (!l.live_[n]) continue;
      ++live;
      require_at(l.live_[n] == MODE || l.live_[n] == DEFERRED, "a live entry is one of the two kinds", line);
      require_at(l.op_[n].parent_clv_index == n, "the operation kept for a node writes that node", line);
      ++users[l.op_[n].child1_matrix_index];
      ++users[l.op_[n].child2_matrix_index];
    }
    require_at(l.count_ == live, "the count equals the live entries", line);
    require_at(l.empty() == (live == 0), "empty() goes by the count", line);
    require_at(users == l.mat_users_, "matrix users equal the live operations that read the matrix", line);
    for (unsigned m = 0; m < users.size(); ++m) require_at(l.matrix_in_use(m) == (users[m] != 0), "matrix_in_use()", line);
    for (int up : l.run_up_) require_at(up >= -1 && up < (int)l.live_.size(), "a link is -1 or a node", line);
  }
};
}
#define INV(l) UnstoredLedgerCheck::invariants((l), __LINE__)

static pll_operation_t op(unsigned parent, unsigned c1, unsigned c2, unsigned m1 = 0, unsigned m2 = 1, int ps = -1,
                          int s1 = -1, int s2 = -1)
{
  pll_operation_t o = pll_operation_t();
  o.parent_clv_index = parent; o.parent_scaler_index = ps;
  o.child1_clv_index = c1; o.child1_matrix_index = m1; o.child1_scaler_index = s1;
  o.child2_clv_index = c2; o.child2_matrix_index = m2; o.child2_scaler_index = s2;
  return o;
}

static UnstoredLedger fresh()
{
  UnstoredLedger l;
  l.reset(NODES, NMAT);
  INV(l);
  require(l.empty() && l.unread_row() == 0);
  return l;
}

// the parents of `ops` given in `nodes`, as a schedule of `kind` leaves them out
static void leave_out(UnstoredLedger & l, const std::vector<pll_operation_t> & ops, const Nodes & nodes, char kind,
                      const Runs & runs = Runs())
{
  l.after_list(ops.data(), (unsigned)ops.size(), nodes, runs, kind);
  INV(l);
}

struct Wants { Nodes want; std::vector<char> going; };
static Wants wants(const UnstoredLedger & l, const std::vector<pll_operation_t> & ops, bool busy = false)
{
  Wants w;
  w.want.assign(3, 77u);                       // (what the call finds there does not matter)
  w.going.assign(2, 1);
  l.before_list(ops.data(), (unsigned)ops.size(), NSCALERS, busy, w.want, w.going);
  return w;
}

// the parents of the list that stores `want`
struct Recomputed { Nodes parents; unsigned ndeferred; };
static Recomputed recompute(const UnstoredLedger & l, const Nodes & want, bool group, const std::vector<char> * going = nullptr)
{
  std::vector<pll_operation_t> ops(1, op(9, 9, 9));
  Recomputed r;
  r.ndeferred = 99;
  l.recompute_list(want, group, going, ops, r.ndeferred);
  for (const pll_operation_t & o : ops) r.parents.push_back(o.parent_clv_index);
  return r;
}

static bool same_counts(const UnstoredLedger & l, unsigned long long skipped, unsigned long long materialized,
                        unsigned long long discarded, unsigned long long deferred, unsigned long long stored_later,
                        unsigned long long given_up)
{
  const pllhip_transient_stats_t & t = l.transient_stats();
  const pllhip_deferred_stats_t & d = l.deferred_stats();
  return t.skipped == skipped && t.materialized == materialized && t.discarded == discarded && d.deferred == deferred &&
         d.stored_later == stored_later && d.given_up == given_up;
}

static void counting()
{
  section = "counting";
  for (char kind : {MODE, DEFERRED})
  {
    const unsigned m = kind == MODE, d = !m;             // which of the two records moves
    UnstoredLedger l = fresh();
    l.mark(op(4, 0, 1, 0, 1), kind); INV(l);
    require(!l.empty() && l.live(4) == kind && l.live(5) == 0 && l.live(NODES) == 0 && l.live(~0u) == 0);
    require(l.matrix_in_use(0) && l.matrix_in_use(1) && !l.matrix_in_use(2));
    require(same_counts(l, m, 0, 0, d, 0, 0));
    l.drop(4, true); INV(l);
    require(l.empty() && l.live(4) == 0 && !l.matrix_in_use(0) && !l.matrix_in_use(1) && !l.matrix_in_use(2));
    require(same_counts(l, m, 0, m, d, 0, d));
    l.drop(4, true); INV(l);                                        // (not live: nothing to count)
    require(same_counts(l, m, 0, m, d, 0, d));
    // a vector that is being stored is not dead
    l.mark(op(5, 4, 2, 2, 2), kind); INV(l);
    require(l.matrix_in_use(2) && !l.matrix_in_use(0));
    l.drop(5, false); INV(l);
    require(l.empty() && !l.matrix_in_use(2) && same_counts(l, 2 * m, 0, m, 2 * d, 0, d));
    // a second mark on a live node: the first operation is dead, under the kind it had
    l.mark(op(4, 0, 1, 0, 1), kind); INV(l);
    l.mark(op(4, 2, 3, 2, 2), m ? DEFERRED : MODE); INV(l);
    require(l.live(4) == (m ? DEFERRED : MODE) && !l.matrix_in_use(0) && !l.matrix_in_use(1) && l.matrix_in_use(2));
    require(m ? same_counts(l, 3, 0, 2, 1, 0, 0) : same_counts(l, 1, 0, 0, 3, 0, 2));
    // what was stored later is counted by kind, and a reset keeps the statistics
    l.stored(2, 5); INV(l);
    require(m ? same_counts(l, 3, 2, 2, 1, 5, 0) : same_counts(l, 1, 2, 0, 3, 5, 2));
    l.reset(NODES, NMAT); INV(l);
    require(l.empty() && l.live(4) == 0 && !l.matrix_in_use(2));
    require(m ? same_counts(l, 3, 2, 2, 1, 5, 0) : same_counts(l, 1, 2, 0, 3, 5, 2));
  }
}

static void before_list_wants()
{
  section = "before_list";
  {
    UnstoredLedger l = fresh();
    const Wants w = wants(l, {op(5, 4, 2)});                        // nothing is unstored: one test, nothing filled
    require(w.want.empty() && w.going.empty());
  }
  UnstoredLedger l = fresh();
  l.mark(op(4, 0, 1), MODE); INV(l);
  {
    const Wants w = wants(l, {op(5, 4, 2)});                        // read by the list
    require(w.want == Nodes({4}) && w.going.size() == NODES && w.going[5] == 1 && w.going[4] == 0);
  }
  {
    const Wants w = wants(l, {op(4, 0, 1), op(5, 4, 2)});           // read only after the list wrote it
    require(w.want.empty() && w.going[4] == 1 && w.going[5] == 1 && w.going[6] == 0);
  }
  {
    const Wants w = wants(l, {op(4, 2, 3)});                        // overwritten: not wanted, going
    require(w.want.empty() && w.going[4] == 1);
  }
  {
    const Wants w = wants(l, {op(5, 4, 2), op(4, 0, 1)});           // read first, overwritten later: wanted and going
    require(w.want == Nodes({4}) && w.going[4] == 1);
  }
  {
    const Wants w = wants(l, {op(5, 4, 2)}, true);                  // a list that stores such vectors wants nothing
    require(w.want.empty() && w.going.empty());
  }
  l = fresh();
  l.mark(op(5, 4, 2, 0, 1, 2, 0, -1), DEFERRED); INV(l);            // (4 itself is stored)
  require(wants(l, {op(4, 0, 1)}).want == Nodes({5}));              // its child vector is overwritten
  require(wants(l, {op(6, 0, 1, 0, 1, 0)}).want == Nodes({5}));     // its child scale buffer is overwritten
  require(wants(l, {op(6, 0, 1, 0, 1, 2)}).want == Nodes({5}));     // its parent scale buffer is overwritten
  require(wants(l, {op(6, 0, 1, 0, 1, 1)}).want.empty());           // another buffer, another vector: left alone
  require(wants(l, {op(6, 0, 1)}).want.empty());
  l = fresh();
  l.mark(op(5, 2, 3, 0, 1, -1, -1, 1), MODE); INV(l);
  require(wants(l, {op(6, 0, 1, 0, 1, 1)}).want == Nodes({5}));     // child 2's scale buffer
  // the order: what the list reads, in list order, then what loses an input, by index (repeats stay)
  l = fresh();
  l.mark(op(4, 0, 1), MODE); INV(l);
  l.mark(op(6, 7, 3), DEFERRED); INV(l);
  l.mark(op(9, 7, 2), MODE); INV(l);
  require(wants(l, {op(8, 6, 4), op(7, 0, 1)}).want == Nodes({6, 4, 6, 9}));
}

static void give_up_written()
{
  section = "give_up_written";
  for (bool busy : {false, true})
  {
    UnstoredLedger l = fresh();
    const std::vector<pll_operation_t> ops = {op(4, 0, 1), op(5, 2, 3, 2, 2), op(6, 4, 5)};
    l.mark(ops[0], DEFERRED); INV(l);
    l.mark(ops[1], MODE); INV(l);
    l.give_up_written(ops.data(), 3, busy); INV(l);
    require(l.empty() && l.live(4) == 0 && l.live(5) == 0);
    require(busy ? same_counts(l, 1, 0, 0, 1, 0, 0) : same_counts(l, 1, 0, 1, 1, 0, 1));
  }
}

static void runs()
{
  section = "runs";
  const std::vector<pll_operation_t> path = {op(4, 0, 1), op(5, 4, 2), op(6, 5, 3)};
  const Runs links = {{4, 5}, {5, 6}};
  auto deferred_path = [&]() { UnstoredLedger l = fresh(); leave_out(l, path, {4, 5, 6}, DEFERRED, links); return l; };
  {
    const UnstoredLedger l = deferred_path();
    Recomputed r = recompute(l, {4}, true);
    require(r.parents == Nodes({4, 5, 6}) && r.ndeferred == 3);      // one list that ends in c's operation
    r = recompute(l, {4}, false);
    require(r.parents == Nodes({4}) && r.ndeferred == 1);            // grouping off: a's alone
    r = recompute(l, {5}, true);
    require(r.parents == Nodes({4, 5, 6}));                          // (what lies below comes along as for every vector)
    std::vector<char> going(NODES, 0);
    going[6] = 1;
    require(recompute(l, {4}, true, &going).parents == Nodes({4, 5})); // not into a vector that is about to go
    going[5] = 1;
    require(recompute(l, {4}, true, &going).parents == Nodes({4}));
  }
  {
    UnstoredLedger l = deferred_path();                              // the upper vector is no longer deferred: stored ...
    l.drop(6, false); INV(l);
    require(recompute(l, {4}, true).parents == Nodes({4, 5}));
    l.mark(op(6, 5, 3), MODE); INV(l);                               // ... or left out by an evaluate-only traversal
    require(recompute(l, {4}, true).parents == Nodes({4, 5}));
  }
  {
    UnstoredLedger l = deferred_path();                              // the upper vector is another operation by now
    l.mark(op(5, 2, 3), DEFERRED); INV(l);
    require(UnstoredLedgerCheck::run_up(l, 4) == 5);                 // (the link is still there, and does not hold)
    const Recomputed r = recompute(l, {4}, true);
    require(r.parents == Nodes({4}) && r.ndeferred == 1);
    require(recompute(l, {5}, true).parents == Nodes({5}));          // ... and the new operation has no link upwards
  }
}

static void recompute_lists()
{
  section = "recompute_list";
  UnstoredLedger l = fresh();
  require(recompute(l, {4}, true).parents.empty() && recompute(l, {4}, true).ndeferred == 0);   // nothing is unstored
  const std::vector<pll_operation_t> ops = {op(4, 0, 1), op(5, 2, 3), op(6, 4, 5), op(7, 4, 3), op(8, 9, 7)};
  leave_out(l, ops, {4, 6, 7}, MODE);
  leave_out(l, ops, {5}, DEFERRED);
  Recomputed r = recompute(l, {6, 7}, true);
  require(r.parents == Nodes({4, 5, 6, 7}) && r.ndeferred == 1);     // children first, the shared child 4 once
  r = recompute(l, {7, 6}, false);
  require(r.parents == Nodes({4, 7, 5, 6}) && r.ndeferred == 1);
  r = recompute(l, {9, 6, 6, NODES, 99, 8, 4}, true);                // not live, repeated, out of range: skipped
  require(r.parents == Nodes({4, 5, 6}) && r.ndeferred == 1);
  r = recompute(l, {8, 9, 12}, true);
  require(r.parents.empty() && r.ndeferred == 0);
  // once that list has run: its vectors were dropped on the way, the statistics follow
  l.give_up_written(ops.data(), 3, true); INV(l);
  l.stored(2, 1); INV(l);
  require(l.live(7) == MODE && l.live(4) == 0 && same_counts(l, 3, 2, 0, 1, 1, 0));
}

static void after_lists()
{
  section = "after_list";
  const std::vector<pll_operation_t> path = {op(4, 0, 1), op(5, 4, 2), op(6, 5, 3)};
  const Runs links = {{4, 5}, {5, 6}};
  auto links_are = [](const UnstoredLedger & l, int a, int b, int c)
  {
    return UnstoredLedgerCheck::run_up(l, 4) == a && UnstoredLedgerCheck::run_up(l, 5) == b &&
           UnstoredLedgerCheck::run_up(l, 6) == c;
  };
  {
    UnstoredLedger l = fresh();
    leave_out(l, path, {5, 8}, DEFERRED, links);                     // only the parents it is given (8 is none of the list)
    require(l.live(4) == 0 && l.live(5) == DEFERRED && l.live(6) == 0 && l.live(8) == 0 && same_counts(l, 0, 0, 0, 1, 0, 0));
    require(links_are(l, -1, -1, -1));                               // a link needs both ends deferred
  }
  {
    UnstoredLedger l = fresh();
    leave_out(l, path, {5, 4}, DEFERRED, links);
    require(l.live(4) == DEFERRED && l.live(5) == DEFERRED && l.live(6) == 0 && links_are(l, 5, -1, -1));
  }
  {
    UnstoredLedger l = fresh();
    l.mark(path[2], MODE); INV(l);                                   // the upper end is unstored, but not deferred
    leave_out(l, path, {4, 5}, DEFERRED, links);
    require(links_are(l, 5, -1, -1));
  }
  {
    UnstoredLedger l = fresh();
    leave_out(l, path, {4, 5, 6}, MODE, links);                      // evaluate-only traversals never set links
    require(l.live(4) == MODE && l.live(5) == MODE && l.live(6) == MODE && links_are(l, -1, -1, -1));
    require(same_counts(l, 3, 0, 0, 0, 0, 0));
    require(recompute(l, {4}, true).parents == Nodes({4}));
    leave_out(l, path, Nodes(), DEFERRED, Runs());                   // a schedule that left nothing out
    require(same_counts(l, 3, 0, 0, 0, 0, 0));
  }
}

static void discard()
{
  section = "discard_mode_vectors";
  UnstoredLedger l = fresh();
  l.mark(op(4, 0, 1), MODE); INV(l);
  l.mark(op(5, 2, 3, 2, 2), DEFERRED); INV(l);
  l.mark(op(6, 4, 5), MODE); INV(l);
  l.discard_mode_vectors(); INV(l);
  require(l.live(4) == 0 && l.live(5) == DEFERRED && l.live(6) == 0 && !l.empty());
  require(l.matrix_in_use(2) && !l.matrix_in_use(0) && same_counts(l, 2, 0, 2, 1, 0, 0));
  l.discard_mode_vectors(); INV(l);
  require(l.live(5) == DEFERRED && same_counts(l, 2, 0, 2, 1, 0, 0));
}

static void row_rule()
{
  section = "row rule";
  UnstoredLedger l = fresh();
  l.deferring_list_ran(); INV(l); require(l.unread_row() == 1);
  l.deferring_list_ran(); INV(l); require(l.unread_row() == 2);
  l.deferring_list_ran(); INV(l); require(l.unread_row() == 3);
  l.stored(3, 0);                 require(l.unread_row() == 3);      // (what evaluate-only traversals left out says nothing)
  l.stored(0, 1);                 require(l.unread_row() == 0);      // a deferred vector was stored: the row is over
  l.deferring_list_ran(); INV(l); require(l.unread_row() == 1);      // ... and the next deferring list starts one
  l.deferring_list_ran(); INV(l); require(l.unread_row() == 2);
  l.stored(0, 2);                 require(l.unread_row() == 0);
  l.stored(0, 1);                 require(l.unread_row() == 0);
  l.deferring_list_ran(); INV(l); require(l.unread_row() == 1);
  l.reset(NODES, NMAT); INV(l);   require(l.unread_row() == 0);
  l.deferring_list_ran(); INV(l); require(l.unread_row() == 1);
}

int main()
{
  counting();
  before_list_wants();
  give_up_written();
  runs();
  recompute_lists();
  after_lists();
  discard();
  row_rule();
  printf("ok\n");
  return 0;
}
