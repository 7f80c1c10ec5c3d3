"""Deferred stores (pll-modules_amd/csrc/pll_core.hip, plan_defers; kernels_s20.hpp, PlanOp::flags bit 0 in the
fold-capable instantiations of k_traverse_s20): a storing traversal of the 20-state family leaves out the stores of
folded cherries and of the chains of looked-up children -- vectors that no operation of the list reads from memory and
that coded tips alone recompute.  The engine keeps such a vector as its operation (the records of evaluate-only
traversals) and stores it for its first reader or before an input changes, so everything a caller can read must be EQUAL
BIT FOR BIT to the same library planning every store (PLLHIP_DEFER=0): every vector through pllhip_get_clv, every scaler
array, the likelihood and the per-site likelihoods -- after a full traversal, after new branch lengths, after a changed
tip, after partial lists that read or overwrite a deferred cherry, after edge likelihoods, sumtables and derivatives at
a deferred cherry, after the ancestral batch, a host round trip, the evaluate-only mode going on and off, and
pllhip_discard_transient.  Any difference is a bug, not rounding.  The deferring run is compared with the CPU oracle as
well, within the suite's tolerances.

PLLHIP_DEFER (1: deferred stores at any partition size -- by default they start at 3840 site blocks --, 0: none),
PLLHIP_LOOKUP (1: class tables at any partition size) and PLLHIP_TRAVERSE (one launch per traversal / one per round
of chains) are read once per process, so each combination runs in a child process
(tests/_defer_worker.py) that takes every case through every checkpoint and writes digests and counters."""
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


@functools.lru_cache(maxsize=None)
def _run(defer, traverse):
    """the worker's results under PLLHIP_DEFER=defer, PLLHIP_TRAVERSE=traverse (the deferring runs also check the oracle)"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "defer.json")
        env = {**os.environ, "PLLHIP_DEFER": str(defer), "PLLHIP_LOOKUP": "1", "PLLHIP_TRAVERSE": str(traverse)}
        env.pop("PLLHIP_LOOKUP_CLASSES", None)
        env.pop("PLLHIP_FOLD", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_defer_worker.py"), out, "1" if defer else "0"],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        with open(out) as f:
            return json.load(f)


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_deferred_stores_change_nothing_a_caller_can_see(product, case, traverse):
    on, off = _run(1, traverse)[case], _run(0, traverse)[case]
    assert on.get("oracle") is True                   # the worker compared this case with the oracle
    assert on["values"].keys() == off["values"].keys()
    diff = [k for k in on["values"] if on["values"][k] != off["values"][k]]
    assert not diff, f"not bit-identical to PLLHIP_DEFER=0: {diff[:8]} ({len(diff)} of {len(on['values'])})"


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_counters_report_the_deferred_stores(product, case, traverse):
    on, off = _run(1, traverse)[case]["counters"], _run(0, traverse)[case]["counters"]
    # the schedule is the same but for the stores: pllhip_schedule_stats keeps its numbers
    assert on["schedule"] == off["schedule"]
    assert off["after_first"] == [0, 0, 0] and off["after_readers"] == [0, 0, 0] and sum(off["per_reader"]) == 0
    # pllhip_transient_stats counts what the mode caused alone: the same with and without deferred stores
    assert on["transient"] == off["transient"]
    if common.FORCED:
        # site repeats and evaluate-only traversals (when the suite forces them) plan as before: nothing is deferred
        assert on["after_first"] == [0, 0, 0] and on["after_readers"] == [0, 0, 0]
        return
    deferred, stored_later, given_up = on["after_first"]
    assert stored_later == 0 and given_up == 0
    if case.startswith("ladder"):
        assert deferred == 0                            # no light cherry: nothing to defer
        return
    assert deferred > 0
    # stored later: exactly the nodes a reader asked for, one each (children come before parents in the reading order)
    assert all(x in (0, 1) for x in on["per_reader"])
    assert sum(on["per_reader"]) == deferred
    assert on["after_readers"] == [deferred, deferred, 0]
    # deferred = the folded cherries + the operations of the looked-up children's chains.  A looked-up child is a
    # cherry (one operation) or a cherry x tip (two: the cherry goes up in registers), so the deferred cherries number
    # folded_cherries + lookup_children, and every other deferred node is a cherry x tip above a deferred cherry
    shape, ntips, _ = CASES[case]
    tree = make_tree(pc, shape, ntips)
    nodes = {op[0]: op for op, x in zip(tree.ops, on["per_reader"]) if x}
    cherries = {n for n, op in nodes.items() if op[2] < ntips and op[5] < ntips}
    sched = on["schedule"]
    assert len(cherries) == sched["folded_cherries"] + sched["lookup_children"]
    for n, op in nodes.items():
        if n not in cherries:
            assert (op[2] < ntips) != (op[5] < ntips) and (op[2] in cherries or op[5] in cherries), op
    # the partial lists read deferred cherries from memory and overwrite others
    assert on["partial_reads"] > 0 and on["partial_overwrites"] > 0


@pytest.mark.parametrize("traverse", [1, 0])
def test_full_evaluations_in_a_row_store_nothing_later(product, traverse):
    """the benchmark's pattern: what one evaluation deferred the next one overwrites before anybody asked -- nothing is
    recomputed between full evaluations, which is what the gain rests on"""
    on, off = _run(1, traverse)["bench"], _run(0, traverse)["bench"]
    assert on["lnl"] == off["lnl"]
    assert on["transient"] == off["transient"]
    assert off["deferred"] == [[0, 0, 0]] * 4
    if common.FORCED:
        assert on["deferred"] == [[0, 0, 0]] * 4
        return
    per_step = on["deferred"][0][0]
    assert per_step > 0
    for step, (deferred, stored_later, given_up) in enumerate(on["deferred"]):
        assert deferred == (step + 1) * per_step
        assert stored_later == 0
        assert given_up == step * per_step
