// The chain planner (pll-modules_amd/csrc/chain_plan.cpp) on the CPU: every case of tests/golden/chain_plans.txt --
// operation lists, per-child LDS costs, limits and deferral policy, each with the complete plan that the planner made
// before it became a module of its own -- is planned again and compared field by field (integers: exactly), and every
// plan is held against the invariants below.  A program of its own, built with -fsanitize=address,undefined
// (tests/test_chain_plan.py).  argv[1]: the fixture file.  Prints "ok".
//
// The file, token by token:
//   list NAME COUNT NODES NSCALERS CODED_BELOW, then COUNT times: op <the eight fields of pll_operation_t>
//   case LIST / costs 0|1 TIP INNER WIDE <LDS doubles of the table of a coded tip, of any other child, of a wide tip; 0:
//   no tables> / wide FLAGS / limits MAX_LEN LDS_CAP FOLD_LDS LOOK_CLASSES LUT_USED DEFER_LEVEL DEFER_DEPTH / accepted
//   0|1, and if accepted: chains N, N times: chain LAUNCH LDS LEN <ops> / rounds R / carried, folded, looked, deferred:
//   FLAGS / lookups N, N times: CONSUMER TOP CHERRY NCLASSES / run_up SIZE PAIRS, PAIRS times: OP UP / order_rounds,
//   order_depth: N <chains> / end.  FLAGS: one digit per operation (wide: per child), "-": an empty array
#include "chain_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>
#include <vector>

using namespace chainplan;

struct List { std::vector<pll_operation_t> ops; unsigned nodes, nscalers, coded_below; };

static std::ifstream in;
static unsigned case_no = 0;
static std::string case_name;

[[noreturn]] static void fail(const char * what)
{
  printf("case %u (%s): %s\n", case_no, case_name.c_str(), what);
  exit(1);
}
static void require(bool ok, const char * what) { if (!ok) fail(what); }

static std::string word() { std::string w; if (!(in >> w)) { printf("fixture file ends early\n"); exit(1); } return w; }
static long number() { long v; if (!(in >> v)) { printf("fixture file: number expected\n"); exit(1); } return v; }
static void expect(const char * w) { if (word() != w) { printf("fixture file: '%s' expected in case %u\n", w, case_no); exit(1); } }
template <class T> static std::vector<T> numbers(const char * name)
{
  expect(name);
  std::vector<T> v((size_t)number());
  for (T & x : v) x = (T)number();
  return v;
}
static std::vector<unsigned char> flags(const char * name)
{
  expect(name);
  const std::string w = word();
  std::vector<unsigned char> v;
  for (char c : w) if (c != '-') v.push_back((unsigned char)(c - '0'));
  return v;
}

// inner vectors that the chains read from memory: neither handed over in registers nor folded into the reader
static unsigned inner_reads(const ListFacts & facts, const ChainPlan & plan)
{
  unsigned n = 0;
  for (unsigned k = 0; k < facts.count(); ++k)
    for (unsigned x = 0; x < 2; ++x)
    {
      const int p = facts.producer[2 * k + x];
      if (p >= 0 && plan.carried[k] != x + 1 && !(!plan.folded.empty() && plan.folded[p])) ++n;
    }
  return n;
}

static void check_invariants(const ChainList & list, const ListFacts & facts, const ChainPlan & plan, unsigned max_len,
                             unsigned lds_cap, unsigned fold_lds)
{
  const unsigned count = list.count;
  auto folded = [&](unsigned k) { return !plan.folded.empty() && plan.folded[k] != 0; };
  std::vector<unsigned> seen(count, 0);
  std::vector<int> next_in_chain(count, -1);
  require(plan.launch.size() == plan.chains.size() && plan.lds.size() == plan.chains.size(), "launch / lds per chain");
  require(plan.carried.size() == count, "carried per operation");
  for (size_t c = 0; c < plan.chains.size(); ++c)
  {
    const std::vector<unsigned> & ch = plan.chains[c];
    unsigned len = 0, lds = 0;
    int before = -1;                                   // the entry before, skipping a folded cherry
    for (size_t i = 0; i < ch.size(); ++i)
    {
      const unsigned k = ch[i];
      require(k < count, "operation index");
      ++seen[k];
      if (i + 1 < ch.size()) next_in_chain[k] = (int)ch[i + 1];
      if (folded(k))
      {
        require(i + 1 < ch.size() && !folded(ch[i + 1]) && facts.consumer[k] == (int)ch[i + 1], "a folded cherry stands in front of its consumer");
        require(facts.producer[2 * ch[i + 1] + plan.folded[k] - 1] == (int)k, "the side of a folded cherry");
        lds += fold_lds;
        continue;
      }
      ++len;
      lds += list.lds(k);
      if (before < 0) require(plan.carried[k] == 0, "the first operation of a chain takes nothing over");
      else require(plan.carried[k] && facts.producer[2 * k + plan.carried[k] - 1] == before, "a carried child is the parent of the entry before");
      before = (int)k;
    }
    require(len >= 1 && len <= max_len, "operations per chain");
    require(lds == plan.lds[c], "LDS doubles of a chain");
    require(lds <= lds_cap || ch.size() == 1, "LDS cap");
  }
  for (unsigned k = 0; k < count; ++k) require(seen[k] == 1, "each operation is in exactly one chain");
  for (unsigned k = 0; k < count && !plan.deferred.empty(); ++k)
  {
    if (!plan.deferred[k]) continue;
    // (a looked-up child ends a chain of its own: its reader takes rows of the class table instead of the vector)
    const int c = facts.consumer[k];
    require(c >= 0, "a deferred vector has a reader in the list");
    if (!plan.looked.empty() && plan.looked[c] && facts.producer[2 * c + plan.looked[c] - 1] == (int)k) continue;
    require(next_in_chain[k] >= 0, "a deferred operation is never the last of its chain");
    const bool in_registers = plan.carried[c] && facts.producer[2 * c + plan.carried[c] - 1] == (int)k;
    require(in_registers || (folded(k) && next_in_chain[k] == c), "a deferred vector is read from memory");
  }
  if (!plan.run_up.empty())
    for (unsigned k = 0; k < count; ++k)
      if (plan.run_up[k] >= 0)
        require(plan.deferred[k] && plan.deferred[plan.run_up[k]] && next_in_chain[k] == plan.run_up[k], "run_up links neighbours that are both deferred");
}

int main(int argc, char ** argv)
{
  if (argc < 2) { printf("usage: chain_plan_host_check <fixture file>\n"); return 2; }
  in.open(argv[1]);
  if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
  std::map<std::string, List> lists;
  unsigned accepted_cases = 0, with_folds = 0, with_lookups = 0, with_defers = 0, with_runs = 0;
  std::string w;
  while (in >> w)
  {
    if (w == "list")
    {
      List & l = lists[word()];
      l.ops.resize((size_t)number());
      l.nodes = (unsigned)number(); l.nscalers = (unsigned)number(); l.coded_below = (unsigned)number();
      for (pll_operation_t & o : l.ops)
      {
        expect("op");
        o.parent_clv_index = (unsigned)number(); o.parent_scaler_index = (int)number();
        o.child1_clv_index = (unsigned)number(); o.child1_matrix_index = (unsigned)number(); o.child1_scaler_index = (int)number();
        o.child2_clv_index = (unsigned)number(); o.child2_matrix_index = (unsigned)number(); o.child2_scaler_index = (int)number();
      }
      continue;
    }
    if (w != "case") { printf("fixture file: unexpected '%s'\n", w.c_str()); return 1; }
    ++case_no;
    case_name = word();
    if (!lists.count(case_name)) fail("unknown list");
    const List & l = lists[case_name];
    // the per-child costs, as the engine fills them: a wide tip's table, a coded tip's, any other child's
    expect("costs");
    const bool tables = number() != 0;
    const unsigned tip_lds = (unsigned)number(), inner_lds = (unsigned)number(), wide_lds = (unsigned)number();
    const std::vector<unsigned char> wide = flags("wide");
    require(wide.empty() || wide.size() == 2 * l.ops.size(), "wide flags per child");
    std::vector<unsigned> costs(tables ? 2 * l.ops.size() : 0);
    for (size_t i = 0; i < costs.size(); ++i)
    {
      const unsigned child = i & 1 ? l.ops[i / 2].child2_clv_index : l.ops[i / 2].child1_clv_index;
      costs[i] = !wide.empty() && wide[i] ? wide_lds : child < l.coded_below ? tip_lds : inner_lds;
    }
    expect("limits");
    const unsigned max_len = (unsigned)number(), lds_cap = (unsigned)number(), fold_lds = (unsigned)number(),
                   look_classes = (unsigned)number(), lut_used = (unsigned)number();
    DeferPolicy policy;
    policy.level = (unsigned)number(); policy.depth = (unsigned)number();
    expect("accepted");
    const bool accepted = number() != 0;

    const ChainList list = {l.ops.data(), (unsigned)l.ops.size(), l.nodes, l.nscalers, l.coded_below, costs.empty() ? nullptr : costs.data()};
    ListFacts facts;
    require(analyse_list(list, facts) == accepted, "acceptance");
    if (accepted)
    {
      ++accepted_cases;
      ChainPlan plan;
      plan_chains(list, facts, max_len, lds_cap, plan);
      check_invariants(list, facts, plan, max_len, lds_cap, fold_lds);
      const unsigned reads_without = inner_reads(facts, plan);
      plan_folds(list, facts, max_len, lds_cap, fold_lds, plan);
      require(inner_reads(facts, plan) <= reads_without, "a plan with folds reads no more inner vectors than the plan without");
      plan_lookups(facts, lut_used, look_classes, plan);
      if (policy.level) plan_defers(facts, policy, plan);
      check_invariants(list, facts, plan, max_len, lds_cap, fold_lds);

      expect("chains");
      require((size_t)number() == plan.chains.size(), "number of chains");
      for (size_t c = 0; c < plan.chains.size(); ++c)
      {
        expect("chain");
        require(number() == plan.launch[c], "launch round of a chain");
        require((unsigned)number() == plan.lds[c], "LDS of a chain");
        require((size_t)number() == plan.chains[c].size(), "length of a chain");
        for (unsigned k : plan.chains[c]) require((unsigned)number() == k, "operations of a chain");
      }
      expect("rounds");
      require(number() == plan.rounds, "rounds");
      require(flags("carried") == plan.carried, "carried");
      require(flags("folded") == plan.folded, "folded");
      require(flags("looked") == plan.looked, "looked");
      require(flags("deferred") == plan.deferred, "deferred");
      expect("lookups");
      require((size_t)number() == plan.lookups.size(), "number of lookups");
      for (const ChainPlan::Lookup & lk : plan.lookups)
      {
        const unsigned consumer = (unsigned)number(), top = (unsigned)number();
        const int cherry = (int)number();
        const unsigned nclasses = (unsigned)number();
        require(consumer == lk.consumer && top == lk.top && cherry == lk.cherry && nclasses == lk.nclasses, "lookup");
      }
      expect("run_up");
      std::vector<int> run_up((size_t)number(), -1);
      for (long pairs = number(); pairs > 0; --pairs) { const size_t k = (size_t)number(); require(k < run_up.size(), "run_up index"); run_up[k] = (int)number(); }
      require(run_up == plan.run_up, "run_up");
      require(numbers<size_t>("order_rounds") == chain_order(facts, plan, true), "chain order by rounds");
      require(numbers<size_t>("order_depth") == chain_order(facts, plan, false), "chain order depth first");
      with_folds += !plan.folded.empty();
      with_lookups += !plan.lookups.empty();
      with_defers += !plan.deferred.empty();
      with_runs += !plan.run_up.empty();
    }
    expect("end");
  }
  // (the corpus is there: a truncated or emptied file does not pass)
  if (case_no < 130 || accepted_cases + 11 != case_no || !with_folds || !with_lookups || !with_defers || !with_runs)
  {
    printf("the corpus is incomplete: %u cases, %u accepted, %u / %u / %u / %u with folds / lookups / deferred stores / runs\n",
           case_no, accepted_cases, with_folds, with_lookups, with_defers, with_runs);
    return 1;
  }
  printf("%u cases, %u accepted, %u / %u / %u / %u with folds / lookups / deferred stores / runs\nok\n",
         case_no, accepted_cases, with_folds, with_lookups, with_defers, with_runs);
  return 0;
}
