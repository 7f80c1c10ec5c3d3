"""Deferred stores, level 4 (pll-modules_amd/csrc/pll_core.hip, plan_defers): next to everything level 3 leaves out, a
storing traversal of the 20-state family leaves out every vector inside a chain that the next operation of the chain
takes in registers and that no other operation of the list reads -- whatever its children are, however far up the chain.
Such a vector is recomputed from stored child vectors and P-matrices, so the engine stores it before one of them
changes.  PLLHIP_DEFER_GROUP=1 lets the reader of a member store the members that stand directly above it in the same
chain in the same list (no folded cherry between them); 0: every reader stores what it reads and what lies below it.

Everything a caller can read must be EQUAL BIT FOR BIT to PLLHIP_DEFER=0 at every checkpoint of _defer_worker.observe,
_defer_runs_worker.observe_runs and _defer_chains_worker.observe_pmat, with the group store on and off, in one launch per
traversal and in one per round of chains; every deferring run is also compared with the CPU oracle within the suite's
tolerances.  The set of deferred nodes, the group store and the benchmark's pattern are checked through
pllhip_deferred_stats.  Every combination of the environment runs in a child process of its own.

Without PLLHIP_DEFER, from the size floor on, the level follows the caller (s20_defer): level 1, level 3 once two lists in
a row have run without a deferred vector being stored later, level 4 once CHAIN_ROW have, level 1 again once a reader asks
for one."""
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
CHAIN_ROW = 4                            # S20_DEFER_CHAIN_ROW (pll_core.hip), as in _defer_chains_worker.py


def _run(defer, group, traverse):
    """the worker's results under PLLHIP_DEFER=defer, PLLHIP_DEFER_GROUP=group, PLLHIP_TRAVERSE=traverse (the deferring
    runs also check the oracle)"""
    if common.FORCED and defer:
        group = 1                            # nothing is deferred under the forced modes: one run stands for all of them
    return _run_worker(defer, group, traverse)


@functools.lru_cache(maxsize=None)
def _run_worker(defer, group, traverse):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "defer_chains.json")
        env = {**os.environ, "PLLHIP_DEFER": str(defer), "PLLHIP_DEFER_DEPTH": "0", "PLLHIP_DEFER_GROUP": str(group),
               "PLLHIP_LOOKUP": "1", "PLLHIP_TRAVERSE": str(traverse)}
        env.pop("PLLHIP_LOOKUP_CLASSES", None)
        env.pop("PLLHIP_FOLD", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_defer_chains_worker.py"), out, "1" if defer else "0"],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        with open(out) as f:
            return json.load(f)


def _reference(traverse):
    return _run(0, 0, traverse)


def _deferred_nodes(case, counters):
    """the nodes whose stores a full traversal deferred (group store off: every reader stores its own node)"""
    shape, ntips, _ = CASES[case]
    tree = make_tree(pc, shape, ntips)
    assert all(x in (0, 1) for x in counters["per_reader"])
    return tree, {op[0] for op, x in zip(tree.ops, counters["per_reader"]) if x}


def _nodes(case, level, traverse):
    return _deferred_nodes(case, _run(level, 0, traverse)[case]["counters"])[1]


def _links(tree, nodes4, nodes2, nodes1):
    """{vector: the deferred vector above it that a reader of it brings along}: two operations that plan_defers marked
    by the chain rule and that stand next to each other in a chain -- the upper one reads the lower one (in registers:
    both are left out), neither is a folded cherry or an operation of a looked-up child (level 1 marks those: the top
    of such a child is the last operation of a chain of its own, the cherry below it feeds that top alone), and no
    folded cherry stands between the two as the upper one's other child"""
    tops = {n for n in nodes1 - nodes2}
    up = {}
    for op in tree.ops:
        for lower, other in ((op[2], op[5]), (op[5], op[2])):
            if lower in nodes4 and op[0] in nodes4 and lower not in nodes1 and other not in nodes2 and op[0] not in tops:
                up[lower] = op[0]
    return up


def _simulate(tree, live, up, order, group):
    """what each reader of `order` stores later: the vector it asks for if that is left out, with the group store the
    linked vectors above it, and every vector below those that is left out (`live` is updated)"""
    by_parent = {op[0]: op for op in tree.ops}
    stored = []
    for n in order:
        if n not in live:
            stored.append(0)
            continue
        w = n
        while group and w in up and up[w] in live:
            w = up[w]
        count, stack = 0, [w]
        while stack:
            x = stack.pop()
            if x not in live:
                continue
            live.discard(x)
            count += 1
            stack += [by_parent[x][2], by_parent[x][5]]
        stored.append(count)
    return stored


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_deferred_chains_change_nothing_a_caller_can_see(product, case, group, traverse):
    on, off = _run(4, group, traverse)[case], _reference(traverse)[case]
    assert on.get("oracle") is True                   # the worker compared this case with the oracle
    assert on["values"].keys() == off["values"].keys()
    diff = [k for k in on["values"] if on["values"][k] != off["values"][k]]
    assert not diff, f"not bit-identical to PLLHIP_DEFER=0: {diff[:8]} ({len(diff)} of {len(on['values'])})"


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_level_4_adds_the_vectors_inside_the_chains(product, case, traverse):
    l4 = _run(4, 0, traverse)[case]["counters"]
    l3, l0 = _run(3, 0, traverse)[case]["counters"], _reference(traverse)[case]["counters"]
    # the schedule is the same but for the stores
    assert l4["schedule"] == l3["schedule"] == l0["schedule"]
    assert l4["transient"] == l0["transient"]
    if common.FORCED:
        # site repeats and evaluate-only traversals (when the suite forces them) plan as before: nothing is deferred
        assert l4["after_first"] == [0, 0, 0] and l4["after_readers"] == [0, 0, 0]
        return
    deferred, stored_later, given_up = l4["after_first"]
    assert stored_later == 0 and given_up == 0
    # after every vector has been read: all of them stored, none given up
    assert l4["after_readers"] == [deferred, deferred, 0]
    tree, nodes4 = _deferred_nodes(case, l4)
    _, nodes3 = _deferred_nodes(case, l3)
    assert len(nodes4) == deferred
    assert nodes3 <= nodes4
    readers = {}
    for op in tree.ops:
        readers.setdefault(op[2], []).append(op[0])
        readers.setdefault(op[5], []).append(op[0])
    unread = [op[0] for op in tree.ops if op[0] not in readers]
    assert unread and not nodes4 & set(unread)          # the two ends of the root edge: nobody in the list reads them
    assert all(len(readers[n]) == 1 for n in nodes4)
    # every vector is read from memory by an operation, left out, or read by nobody in the list
    sched = l4["schedule"]
    assert deferred == sched["operations"] - sched["inner_reads"] - len(unread)
    if case == "random40_4100":
        # beyond level 3: a vector inside a chain whose operation reads an inner child next to the handed-over one
        by_parent = {op[0]: op for op in tree.ops}
        assert any(by_parent[n][2] >= tree.ntips and by_parent[n][5] >= tree.ntips for n in nodes4 - nodes3)


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_a_changed_pmatrix_under_a_chain_vector(product, case, group, traverse):
    """the vector of an operation with an inner child is read after the P-matrix towards that child has changed: the
    engine stored it before the matrix changed (the value is part of the bitwise comparison above)"""
    if common.FORCED:
        return                                          # nothing is deferred under the forced modes
    records = _run(4, group, traverse)[case]["counters"]["pmat"]
    tree, nodes4 = _deferred_nodes(case, _run(4, 0, traverse)[case]["counters"])
    nodes3 = _nodes(case, 3, traverse)
    by_parent = {op[0]: op for op in tree.ops}
    hit = 0
    for r in records:
        n = r["node"]
        assert by_parent[n][2] >= tree.ntips or by_parent[n][5] >= tree.ntips
        rose = r["changed"][1] - r["before"][1]
        if n in nodes4:
            assert rose >= 1, r                         # stored before the matrix changed ...
            assert r["read"] == r["changed"], r         # ... and not again for the reader
            hit += n not in nodes3
        assert r["changed"][2] == r["before"][2], r     # nothing is given up by a changed matrix
    if case == "random40_4100":
        assert hit


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_group_store_brings_the_members_above(product, case, traverse):
    if common.FORCED:
        return                                          # nothing is deferred under the forced modes
    single, grouped = _run(4, 0, traverse)[case]["counters"], _run(4, 1, traverse)[case]["counters"]
    tree, nodes4 = _deferred_nodes(case, single)
    nodes3, nodes2, nodes1 = (_nodes(case, level, traverse) for level in (3, 2, 1))
    up = _links(tree, nodes4, nodes2, nodes1)
    assert grouped["after_first"] == single["after_first"]
    # the probes read every caterpillar bottom-up after ONE full traversal, one reader at a time
    order = [n for p in single["runs"]["probes"] for n in p["nodes"]]
    want_single = _simulate(tree, set(nodes4), up, order, False)
    want_grouped = _simulate(tree, set(nodes4), up, order, True)
    assert [x for p in single["runs"]["probes"] for x in p["stored_later"]] == want_single
    assert [x for p in grouped["runs"]["probes"] for x in p["stored_later"]] == want_grouped
    # one reader, one store (the vectors below a reader are stored by then: they are read first)
    assert want_single == [1 if n in nodes4 else 0 for n in order]
    if case in ("ladder20_1031", "random40_4100"):
        assert any(p["stored_later"][0] >= 2 for p in grouped["runs"]["probes"])    # a bottom cherry brought members along
    # every vector read in post-order after a full traversal: a reader brings the members above it along, whatever
    # their children are
    post = [op[0] for op in tree.ops]
    assert grouped["per_reader"] == _simulate(tree, set(nodes4), up, post, True)
    if case == "random40_4100":
        assert any(up[n] not in nodes3 for n in up)     # ... one of which level 3 does not leave out
        assert max(grouped["per_reader"]) >= 2
    # read in post-order, every node still ends up stored exactly once
    assert sum(grouped["per_reader"]) == grouped["after_first"][0]
    assert grouped["after_readers"] == single["after_readers"]


@pytest.mark.parametrize("traverse", [1, 0])
def test_full_evaluations_in_a_row_store_nothing_later(product, traverse):
    """the benchmark's pattern: what one evaluation deferred the next one overwrites before anybody asked"""
    on, l3, off = _run(4, 1, traverse)["bench"], _run(3, 0, traverse)["bench"], _reference(traverse)["bench"]
    assert on["lnl"] == off["lnl"]
    assert on["transient"] == off["transient"]
    assert off["deferred"] == [[0, 0, 0]] * 4
    if common.FORCED:
        assert on["deferred"] == [[0, 0, 0]] * 4
        return
    per_step = on["deferred"][0][0]
    assert per_step > l3["deferred"][0][0] > 0
    for step, (deferred, stored_later, given_up) in enumerate(on["deferred"]):
        assert deferred == (step + 1) * per_step
        assert stored_later == 0
        assert given_up == step * per_step


@functools.lru_cache(maxsize=None)
def _run_adaptive(defer):
    """the worker's `adaptive` checkpoint with PLLHIP_DEFER unset (None) or set"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "adaptive.json")
        env = {k: v for k, v in os.environ.items() if k not in ("PLLHIP_DEFER", "PLLHIP_DEFER_DEPTH", "PLLHIP_DEFER_GROUP",
                                                                 "PLLHIP_LOOKUP", "PLLHIP_LOOKUP_CLASSES", "PLLHIP_FOLD")}
        if defer is not None:
            env["PLLHIP_DEFER"] = str(defer)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_defer_chains_worker.py"), out, "0", "adaptive"],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        with open(out) as f:
            return json.load(f)["adaptive"]


def test_the_default_level_goes_one_step_further(product):
    """CHAIN_ROW + 2 evaluations, every vector read, CHAIN_ROW + 2 evaluations: the first two of a row plan level 1, the
    ones up to the CHAIN_ROW-th level 3, the ones behind them level 4; a vector stored for a reader takes the next lists
    back to level 1.  Nothing a caller reads changes"""
    auto, l0 = _run_adaptive(None), _run_adaptive(0)
    l1, l3, l4 = _run_adaptive(1), _run_adaptive(3), _run_adaptive(4)
    n = CHAIN_ROW + 2
    assert auto["lnl"] == l0["lnl"] == l1["lnl"] == l3["lnl"] == l4["lnl"]
    assert auto["read"] == l0["read"] == l1["read"] == l3["read"] == l4["read"]
    assert l0["deferred"] == [[0, 0, 0]] * (2 * n)
    if common.FORCED:
        assert auto["deferred"] == [[0, 0, 0]] * (2 * n)
        return
    a, b, c = l1["deferred"][0][0], l3["deferred"][0][0], l4["deferred"][0][0]      # per traversal at level 1 / 3 / 4
    assert 0 < a < b < c
    assert [x[0] for x in l4["deferred"]] == [c * k for k in range(1, 2 * n + 1)]
    per_step = [y[0] - x[0] for x, y in zip([[0, 0, 0]] + auto["deferred"], auto["deferred"])]
    row = [a, a] + [b] * (CHAIN_ROW - 2) + [c, c]
    assert per_step == row + row
    # the vectors of the last traversal of the first row were read, every other traversal's overwritten unread
    assert [x[1] for x in auto["deferred"]] == [0] * n + [c] * n
    given_up = [sum(per_step[:k]) - (c if k >= n else 0) for k in range(2 * n)]
    assert [x[2] for x in auto["deferred"]] == given_up
