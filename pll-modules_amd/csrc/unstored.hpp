// The ledger of unstored vectors: vectors that exist "as their operation only".  An evaluate-only traversal
// (pllhip_set_transient) may hand the vectors inside its chains on in registers without storing them, and a storing
// traversal may defer the store of a vector that none of its operations reads from memory (plan_defers).  Such a vector
// stays recomputable -- the operation that made it is kept here -- and is stored for the first reader that needs it, or
// before one of its inputs (child vectors, scale buffers, matrices) changes.
//
// Index logic over pll_operation_t alone: the ledger knows nothing of the engine, of devices or of the environment, and
// builds with any C++17 compiler (tests/unstored_host_check.cpp runs it under ASan + UBSan against written-out cases).
// The engine checks the indices of every list before it comes here, runs the lists the ledger asks for and tells it
// what became of them.
//
// What holds between any two calls:
//   1. the count of unstored vectors equals the number of non-zero entries of live_;
//   2. mat_users_[m] equals the number of live operations that read matrix m (an operation that reads it through both
//      children counts twice);
//   3. run_up_[a] = b is a hint, not a fact: it is followed only while a and b are both still deferred stores and the
//      operation kept for b still takes a as a child (and b is not about to be overwritten).  Nothing clears a link
//      when b is dropped or marked anew; the walk of recompute_list tests it every time.
#pragma once
#include "pll.h"
#include "pllhip.h"
#include <utility>
#include <vector>

namespace unstored {

// why a vector exists as its operation only: an evaluate-only traversal left it out, or a storing traversal deferred
// its store; the two are counted apart (pllhip_transient_stats / pllhip_deferred_stats)
constexpr char TRANSIENT_MODE = 1, TRANSIENT_DEFERRED = 2;

class UnstoredLedger
{
public:
  // sizes the arrays and forgets every vector and the row of deferring lists; the statistics stay
  void reset(unsigned nodes, unsigned nmat);

  bool empty() const { return !count_; }
  char live(unsigned node) const { return node < live_.size() ? live_[node] : 0; }     // 0, or the kind
  bool matrix_in_use(unsigned m) const { return mat_users_[m] != 0; }

  // the parent vector of `op` was left out (an unstored vector it replaces is counted dead)
  void mark(const pll_operation_t & op, char kind);
  // the vector of `node` stops being its operation only: it is being stored (dead = false) or replaced / given up
  void drop(unsigned node, bool dead);

  // Before an operation list runs.  want: the unstored vectors to store first -- those the list reads before it writes
  // them, in list order, then those whose child vector, child scale buffer or parent scale buffer the list overwrites,
  // by index; going: [nodes] the vectors the list overwrites (empty: nothing is unstored, or busy).  busy: the list is
  // itself one that stores such vectors, and wants nothing.
  void before_list(const pll_operation_t * ops, unsigned count, unsigned nscalers, bool busy,
                   std::vector<unsigned> & want, std::vector<char> & going) const;
  // ... and once `want` is stored: what the list overwrites is given up (busy: it is being stored instead)
  void give_up_written(const pll_operation_t * ops, unsigned count, bool busy)
  { for (unsigned k = 0; k < count && count_; ++k) drop(ops[k].parent_clv_index, !busy); }

  // The list that stores the vectors of `want`: the operations that made them and, below them, the ones of the
  // children that were not stored either -- children before parents, each operation once.  group: a deferred vector
  // brings the members of its run above it along (invariant 3; going: not into these, null: none), so that one list
  // stores the run instead of one list per member.  Entries of want that are not live, repeat or are out of range
  // are skipped.  out_ndeferred: how many operations of the list are deferred stores.
  void recompute_list(const std::vector<unsigned> & want, bool group, const std::vector<char> * going,
                      std::vector<pll_operation_t> & out_ops, unsigned & out_ndeferred) const;
  // that list has run (it dropped its vectors on the way, as every list does)
  void stored(unsigned n_mode, unsigned n_deferred)
  { stats_mode_.materialized += n_mode; stats_deferred_.stored_later += n_deferred; }

  // After the launches of a schedule that left vectors out: left_out_parents = their indices, in schedule order (the
  // ones that are no parent of `ops` are ignored); runs = (vector, the vector above it in the same chain) of a
  // deferring schedule.  A link is set where both ends ended up deferred; kind TRANSIENT_MODE sets none.
  void after_list(const pll_operation_t * ops, unsigned count, const std::vector<unsigned> & left_out_parents,
                  const std::vector<std::pair<unsigned, unsigned>> & runs, char kind);

  // the caller discards what evaluate-only traversals left out (a deferred store is not the caller's doing: it stays)
  void discard_mode_vectors();

  // How the caller has treated deferred vectors lately: the lists in a row that deferred stores with no deferred
  // vector stored since the end of the first of them (0: none yet, or one was stored since the last of them).
  void deferring_list_ran()
  { row_ = row_ && stats_deferred_.stored_later == row_mark_ ? row_ + 1u : 1u; row_mark_ = stats_deferred_.stored_later; }
  unsigned unread_row() const { return stats_deferred_.stored_later == row_mark_ ? row_ : 0u; }

  const pllhip_transient_stats_t & transient_stats() const { return stats_mode_; }
  const pllhip_deferred_stats_t & deferred_stats() const { return stats_deferred_; }

private:
  friend struct UnstoredLedgerCheck;            // tests/unstored_host_check.cpp holds the fields against the invariants
  unsigned count_ = 0;                          // vectors that exist as their operation only
  std::vector<char> live_;                      // [nodes] 0, or the kind
  std::vector<pll_operation_t> op_;             // [nodes] what recomputes the vector
  std::vector<int> run_up_;                     // [nodes] the vector above it in the same deferred run (-1: none)
  std::vector<unsigned> mat_users_;             // [nmat]
  pllhip_transient_stats_t stats_mode_ = {};
  pllhip_deferred_stats_t stats_deferred_ = {}; // the same records, for the stores that storing traversals defer
  unsigned row_ = 0;
  unsigned long long row_mark_ = 0;             // stored_later at the end of the last deferring list
};

} // namespace unstored
