// The chain planner: how an operation list becomes chains, folds, class-table reads and deferred stores.  Host
// combinatorics on indices alone: it knows nothing of the engine, of devices or of the environment, and builds with any
// C++17 compiler (tests/chain_plan_host_check.cpp runs it under ASan + UBSan against recorded plans).  The engine
// describes the list (ChainList), decides the limits and the policy, and turns the plan into a schedule.
#pragma once
#include "pll.h"
#include <cstddef>
#include <vector>

namespace chainplan {

// The planner's input.  The indices of `ops` are in range (the engine checks them when it takes the list).
struct ChainList
{
  const pll_operation_t * ops;
  unsigned count;
  unsigned nodes, nscalers;                      // vectors and scale buffers of the partition
  unsigned coded_below;                          // a child with a smaller index is a coded tip (0: tips are not coded)
  const unsigned * child_lds;                    // [2 * count] LDS doubles of the table of child 1 / 2 (null: no tables)
  unsigned lds(unsigned k) const { return child_lds ? child_lds[2 * k] + child_lds[2 * k + 1] : 0u; }
};

// Which stores a storing schedule leaves out (plan_defers): 0 = none, 1 = those of folded cherries and of looked-up
// children, 2 = those of folded cherries alone, 3 = level 1 and the tip-only runs at the bottom of the chains, 4 = level
// 3 and the vectors inside the chains.  depth (level 3): the most operations of a run that are left out (0: all).
struct DeferPolicy { unsigned level = 0, depth = 0; };

// What every stage needs to know of a list, from one pass over it (analyse_list).  All per operation.
struct ListFacts
{
  std::vector<int> producer;                     // [2 * count] the operation that makes child 1 / 2 (-1: none of the list)
  std::vector<int> consumer;                     // the operation that reads the parent vector (-1: none)
  std::vector<unsigned> readers;                 // readers of the parent vector in the list
  std::vector<unsigned> size;                    // operations of the subtree
  std::vector<unsigned char> heavy;              // 1 / 2: the child with the larger subtree, which continues a chain (0: none)
  std::vector<unsigned char> plain;              // bit 0 / 1: child 1 / 2 is a coded tip without a scale buffer
  unsigned count() const { return (unsigned)consumer.size(); }
  bool cherry(unsigned k) const { return plain[k] == 3; }
  int heavy_producer(unsigned k) const { return heavy[k] ? producer[2 * k + heavy[k] - 1] : -1; }
  int light_producer(unsigned k) const { return heavy[k] ? producer[2 * k + 2 - heavy[k]] : -1; }
};

// Chain schedule of an operation list.
struct ChainPlan
{
  std::vector<std::vector<unsigned>> chains;     // op indices, bottom to top
  std::vector<int> launch;                       // per chain: launch round
  std::vector<unsigned> lds;                     // per chain: LDS doubles of its operations' tables
  std::vector<unsigned char> carried;            // per op
  // per op: 1 / 2 = a lone cherry that the next operation of its chain builds in registers as its child 1 / 2
  // (plan_folds; empty: no folds).  Such an operation sits in front of its consumer in `chains`
  std::vector<unsigned char> folded;
  // children that their consumer reads through a class table instead of the stored vector (plan_lookups), and per op
  // which child that is (1 / 2; empty: none)
  struct Lookup
  {
    unsigned consumer, top;                      // the operation that reads the child; the one that makes it
    int cherry;                                  // top is cherry x tip: the cherry's operation (-1: top is the cherry)
    unsigned nclasses;
  };
  std::vector<Lookup> lookups;
  std::vector<unsigned char> looked;
  // per op: the traversal does not store the parent vector (plan_defers; empty: every vector is stored)
  std::vector<unsigned char> deferred;
  // per op: the operation above it in the same deferred chain-bottom run (-1: none; empty: no such runs)
  std::vector<int> run_up;
  int rounds = 0;
};

// false: the list does not have the shape of a tree traversal -- every vector written once, read by at most one later
// operation, nothing overwritten after it was read, child scalers being the ones the producers wrote --, and `facts`
// is not to be used.
bool analyse_list(const ChainList & list, ListFacts & facts);

// The stages, in this order; `facts`: analyse_list's, of an accepted list.
void plan_chains(const ChainList & list, const ListFacts & facts, unsigned max_len, unsigned lds_cap, ChainPlan & plan);
void plan_folds(const ChainList & list, const ListFacts & facts, unsigned max_len, unsigned lds_cap, unsigned fold_lds,
                ChainPlan & plan);
void plan_lookups(const ListFacts & facts, unsigned lut_used, unsigned max_classes, ChainPlan & plan);
void plan_defers(const ListFacts & facts, DeferPolicy policy, ChainPlan & plan);

std::vector<size_t> chain_order(const ListFacts & facts, const ChainPlan & plan, bool by_rounds);

} // namespace chainplan
