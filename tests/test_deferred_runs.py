"""Deferred stores, level 3 (pll-modules_amd/csrc/pll_core.hip, plan_defers): next to the folded cherries and the chains of
looked-up children a storing traversal of the 20-state family leaves out the tip-only run at the bottom of every chain --
the cherry a chain starts with and the "handed-over child x coded tip" operations above it, as long as the next operation
of the chain takes the result in registers.  PLLHIP_DEFER_DEPTH=D caps such a run at D operations (0: no cap);
PLLHIP_DEFER_GROUP=1 lets the first reader of a member store the whole run as one list (0: every reader stores what it
reads and what lies below it).  A schedule that defers but has neither folds nor looked-up children (a caterpillar) runs
the evaluate-only instantiation of k_traverse_s20, the one without folds that reads PlanOp::flags bit 0.

Everything a caller can read must be EQUAL BIT FOR BIT to PLLHIP_DEFER=0 at every checkpoint of _defer_worker.observe and
of _defer_runs_worker.observe_runs, for D = 1, 2 and no cap, with the group store on and off, in one launch per traversal
and in one per round of chains; every deferring run is also compared with the CPU oracle within the suite's tolerances.
The set of deferred nodes, the group store, partial lists above a run and the benchmark's pattern are checked through
pllhip_deferred_stats.  Every combination of the environment runs in a child process of its own.

Without PLLHIP_DEFER, from the size floor on, the level follows the caller (s20_defer): level 1 until two lists in a row
have run without a deferred vector being stored later, level 3 from then on, level 1 again once a reader asks for one."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import pytest

import common
import pllhip_ctypes as pc
from _defer_worker import CASES, make_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = [1, 2, 0]                       # 0: the whole run


def _run(defer, depth, group, traverse):
    """the worker's results under PLLHIP_DEFER=defer, PLLHIP_DEFER_DEPTH=depth, PLLHIP_DEFER_GROUP=group,
    PLLHIP_TRAVERSE=traverse (the deferring runs also check the oracle)"""
    if common.FORCED and defer:
        depth, group = 0, 1                  # nothing is deferred under the forced modes: one run stands for all of them
    return _run_worker(defer, depth, group, traverse)


@functools.lru_cache(maxsize=None)
def _run_worker(defer, depth, group, traverse):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "defer_runs.json")
        env = {**os.environ, "PLLHIP_DEFER": str(defer), "PLLHIP_DEFER_DEPTH": str(depth), "PLLHIP_DEFER_GROUP": str(group),
               "PLLHIP_LOOKUP": "1", "PLLHIP_TRAVERSE": str(traverse)}
        env.pop("PLLHIP_LOOKUP_CLASSES", None)
        env.pop("PLLHIP_FOLD", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_defer_runs_worker.py"), out, "1" if defer else "0"],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        with open(out) as f:
            return json.load(f)


def _reference(traverse):
    return _run(0, 0, 0, traverse)


def _level1(traverse):
    return _run(1, 0, 0, traverse)


def _deferred_nodes(case, counters):
    """the nodes whose stores a full traversal deferred (group store off: every reader stores its own node)"""
    shape, ntips, _ = CASES[case]
    tree = make_tree(pc, shape, ntips)
    assert all(x in (0, 1) for x in counters["per_reader"])
    return tree, {op[0] for op, x in zip(tree.ops, counters["per_reader"]) if x}


def _run_members(probe_nodes, extra):
    """of a caterpillar (bottom-up), the members of its deferred run: its first operations that level 3 added"""
    run = []
    for n in probe_nodes:
        if n not in extra:
            break
        run.append(n)
    return run


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_deferred_runs_change_nothing_a_caller_can_see(product, case, depth, group, traverse):
    on, off = _run(3, depth, group, traverse)[case], _reference(traverse)[case]
    assert on.get("oracle") is True                   # the worker compared this case with the oracle
    assert on["values"].keys() == off["values"].keys()
    diff = [k for k in on["values"] if on["values"][k] != off["values"][k]]
    assert not diff, f"not bit-identical to PLLHIP_DEFER=0: {diff[:8]} ({len(diff)} of {len(on['values'])})"


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_level_3_adds_the_runs_at_the_bottom_of_chains(product, case, depth, traverse):
    l3 = _run(3, depth, 0, traverse)[case]["counters"]
    l1, l0 = _level1(traverse)[case]["counters"], _reference(traverse)[case]["counters"]
    # the schedule is the same but for the stores
    assert l3["schedule"] == l1["schedule"] == l0["schedule"]
    assert l3["transient"] == l0["transient"]
    if common.FORCED:
        # site repeats and evaluate-only traversals (when the suite forces them) plan as before: nothing is deferred
        assert l3["after_first"] == [0, 0, 0] and l3["after_readers"] == [0, 0, 0]
        return
    deferred, stored_later, given_up = l3["after_first"]
    assert stored_later == 0 and given_up == 0
    # after every vector has been read: all of them stored, none given up
    assert l3["after_readers"] == [deferred, deferred, 0]
    tree, nodes3 = _deferred_nodes(case, l3)
    _, nodes1 = _deferred_nodes(case, l1)
    assert len(nodes3) == deferred
    assert nodes1 <= nodes3
    if case.startswith("ladder"):
        assert not nodes1 and nodes3                    # no light cherry, but a chain that starts with a cherry
        assert l3["schedule"]["folded_cherries"] == 0 and l3["schedule"]["lookup_children"] == 0
    # every node that level 3 adds is the top of a caterpillar: a cherry of tips, then operations with exactly one tip
    # child, `depth` operations at the most
    by_parent = {op[0]: op for op in tree.ops}
    readers = {}
    for op in tree.ops:
        readers.setdefault(op[2], []).append(op[0])
        readers.setdefault(op[5], []).append(op[0])
    for n in nodes3 - nodes1:
        length, op = 1, by_parent[n]
        while not (op[2] < tree.ntips and op[5] < tree.ntips):
            assert (op[2] < tree.ntips) != (op[5] < tree.ntips), (n, op)
            op = by_parent[op[5] if op[2] < tree.ntips else op[2]]
            assert op[0] in nodes3, (n, op)             # a run is deferred from its cherry upwards
            length += 1
        assert not depth or length <= depth, (n, length)
        assert len(readers.get(n, [])) == 1             # one operation takes it (in registers); the root's never go
    if depth != 1 and case in ("ladder20_1031", "random40_4100"):
        assert any(len(_run_members(p["nodes"], nodes3 - nodes1)) >= 2 for p in l3["runs"]["probes"])


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_group_store_brings_the_whole_run(product, case, depth, traverse):
    if common.FORCED:
        return                                          # nothing is deferred under the forced modes
    single, grouped = _run(3, depth, 0, traverse)[case]["counters"], _run(3, depth, 1, traverse)[case]["counters"]
    _, nodes3 = _deferred_nodes(case, single)
    _, nodes1 = _deferred_nodes(case, _level1(traverse)[case]["counters"])
    extra = nodes3 - nodes1
    assert grouped["after_first"] == single["after_first"]
    seen = 0
    for one, all_ in zip(single["runs"]["probes"], grouped["runs"]["probes"]):
        assert one["nodes"] == all_["nodes"]
        run = _run_members(one["nodes"], extra)
        # one reader, one store (the vectors below a reader are stored by then: they are read first)
        assert one["stored_later"] == [1 if n in nodes3 else 0 for n in one["nodes"]]
        if len(run) >= 2:
            seen += 1
            want = [len(run)] + [0] * (len(run) - 1) + [1 if n in nodes3 else 0 for n in one["nodes"][len(run):]]
            assert all_["stored_later"] == want, (run, all_)
        else:
            assert all_["stored_later"] == one["stored_later"]      # level-1 vectors keep one store per reader
    if depth != 1 and case in ("ladder20_1031", "random40_4100"):
        assert seen
    # read in post-order, every node still ends up stored exactly once
    assert sum(grouped["per_reader"]) == grouped["after_first"][0]
    assert grouped["after_readers"] == single["after_readers"]


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("case", ["ladder20_1031", "random40_4100"])
def test_a_partial_list_above_a_run(product, case, depth, group, traverse):
    """the list towards the pendant edge of a tip inside a run reads the members below that tip from memory and overwrites
    the ones above: the former are stored first (with whatever deferred vector lies below them), the latter given up
    unstored -- the values are part of the bitwise comparison above, the counters are checked here"""
    if common.FORCED:
        return                                          # nothing is deferred under the forced modes
    counters = _run(3, depth, group, traverse)[case]["counters"]
    tree, nodes3 = _deferred_nodes(case, _run(3, depth, 0, traverse)[case]["counters"])
    by_parent = {op[0]: op for op in tree.ops}

    def live_below(n):
        return 0 if n not in nodes3 else 1 + live_below(by_parent[n][2]) + live_below(by_parent[n][5])

    partials = counters["runs"]["partials"]
    assert partials
    hit = 0
    for p in partials:
        written = set(p["written"])
        assert set(p["nodes"][p["member"]:]) <= written and not set(p["nodes"][:p["member"]]) & written
        assert p["nodes"][p["member"] - 1] in p["read"]
        stored = sum(live_below(n) for n in p["read"])
        given_up = len(nodes3 & written)
        hit += len(nodes3 & set(p["nodes"]))
        # (the counters run on from the checkpoints before; `before` is taken after a fresh full traversal)
        # (the list is a schedule of its own and may defer stores of its own: a chain of it that starts with a cherry)
        after = [x - y for x, y in zip(p["after"], p["before"])]
        assert after[0] >= 0 and after[1:] == [stored, given_up], p
        # ... and after every vector has been read, every deferred vector was either stored or given up
        end = [x - y for x, y in zip(p["end"], p["before"])]
        assert end[0] == after[0] and end[1] + end[2] == len(nodes3) + end[0], p
    assert hit


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("depth", DEPTHS)
def test_full_evaluations_in_a_row_store_nothing_later(product, depth, traverse):
    """the benchmark's pattern: what one evaluation deferred the next one overwrites before anybody asked"""
    on, l1, off = _run(3, depth, 1, traverse)["bench"], _level1(traverse)["bench"], _reference(traverse)["bench"]
    assert on["lnl"] == off["lnl"]
    assert on["transient"] == off["transient"]
    assert off["deferred"] == [[0, 0, 0]] * 4
    if common.FORCED:
        assert on["deferred"] == [[0, 0, 0]] * 4
        return
    per_step = on["deferred"][0][0]
    assert per_step > l1["deferred"][0][0] > 0
    for step, (deferred, stored_later, given_up) in enumerate(on["deferred"]):
        assert deferred == (step + 1) * per_step
        assert stored_later == 0
        assert given_up == step * per_step


@pytest.mark.parametrize("traverse", [1, 0])
def test_a_schedule_without_folds_still_leaves_its_stores_out(product, traverse):
    """a caterpillar has neither folds nor looked-up children: its deferring schedule must run an instantiation that reads
    PlanOp::flags bit 0 (the plain storing one writes the vectors and the engine would store them a second time)"""
    on, off = _run(3, 0, 1, traverse)["ladder20_1031"], _reference(traverse)["ladder20_1031"]
    assert on["counters"]["schedule"]["folded_cherries"] == 0 and on["counters"]["schedule"]["lookup_children"] == 0
    assert on["values"] == off["values"]
    if not common.FORCED:
        assert on["counters"]["after_first"][0] > 0


@functools.lru_cache(maxsize=None)
def _run_adaptive(defer):
    """the worker's `adaptive` checkpoint with PLLHIP_DEFER unset (None) or set"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "adaptive.json")
        env = {k: v for k, v in os.environ.items() if k not in ("PLLHIP_DEFER", "PLLHIP_DEFER_DEPTH", "PLLHIP_DEFER_GROUP",
                                                                 "PLLHIP_LOOKUP", "PLLHIP_LOOKUP_CLASSES", "PLLHIP_FOLD")}
        if defer is not None:
            env["PLLHIP_DEFER"] = str(defer)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_defer_runs_worker.py"), out, "0", "adaptive"],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        with open(out) as f:
            return json.load(f)["adaptive"]


def test_the_default_level_follows_what_the_caller_reads(product):
    """four evaluations, every vector read, three evaluations: the first two of a row plan level 1, the ones behind them
    level 3; a vector stored for a reader takes the next lists back to level 1.  Nothing a caller reads changes"""
    auto, l0, l1, l3 = _run_adaptive(None), _run_adaptive(0), _run_adaptive(1), _run_adaptive(3)
    assert auto["lnl"] == l0["lnl"] == l1["lnl"] == l3["lnl"]
    assert auto["read"] == l0["read"] == l1["read"] == l3["read"]
    assert l0["deferred"] == [[0, 0, 0]] * 7
    if common.FORCED:
        assert auto["deferred"] == [[0, 0, 0]] * 7
        return
    a, b = l1["deferred"][0][0], l3["deferred"][0][0]             # per traversal at level 1 / 3
    assert 0 < a < b
    assert [x[0] for x in l1["deferred"]] == [a * k for k in range(1, 8)]
    assert [x[0] for x in l3["deferred"]] == [b * k for k in range(1, 8)]
    per_step = [y[0] - x[0] for x, y in zip([[0, 0, 0]] + auto["deferred"], auto["deferred"])]
    assert per_step == [a, a, b, b, a, a, b]
    # the fourth traversal's vectors were read, every other traversal's overwritten unread
    assert [x[1] for x in auto["deferred"]] == [0, 0, 0, 0, b, b, b]
    assert [x[2] for x in auto["deferred"]] == [0, a, 2 * a, 2 * a + b, 2 * a + b, 3 * a + b, 4 * a + b]
