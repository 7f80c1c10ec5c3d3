"""The order inside one operation of a 20-state chain (pll-modules_amd/csrc/kernels_s20.hpp, s20_chain_op): the loads of
an operation go out first, the product of the handed-over child runs under them in place, then the other child's term is
multiplied in.  The factors are the ones of the old order, so every number must be EQUAL BIT FOR BIT to what the
per-operation kernel k_partials_s20 computes (PLLHIP_CHAINS=0: that kernel does not go through s20_chain_op): every inner
vector, every scale buffer, the per-site likelihoods and the likelihood, for every kind of operation -- tip x carried,
inner x carried on either side, folded cherries, class-table children of both kinds, wide tips (site repeats), vector
tips, per-rate scalers, evaluate-only traversals --, with one, two and four rates, at 95 sites (three blocks, the last
one partial) and 33.  Every chain run is also compared with the CPU oracle within the tolerances of
tests/test_gpu_parity.py.  Every combination of the environment runs in a child process of its own
(tests/_chain_op_order_worker.py)."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import pytest

import common
from _chain_op_order_worker import CASES, PLANNED, PLANNED_NO_FOLDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _run(chains, fold, defer, traverse):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "chain_op_order.json")
        env = {**os.environ, "PLLHIP_CHAINS": str(chains), "PLLHIP_LOOKUP": "1", "PLLHIP_FOLD": str(fold),
               "PLLHIP_DEFER": str(defer), "PLLHIP_DEFER_DEPTH": "0", "PLLHIP_TRAVERSE": str(traverse)}
        env.pop("PLLHIP_LOOKUP_CLASSES", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_chain_op_order_worker.py"), out, str(chains)],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        with open(out) as f:
            return json.load(f)


def _reference():
    """the per-operation kernel: no chains, so nothing is folded, looked up, deferred or traversed in one launch"""
    return _run(0, 0, 0, 0)


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("defer", [0, 3, 4])
@pytest.mark.parametrize("fold", [1, 0])
def test_chain_operations_equal_the_per_operation_kernel_bitwise(product, fold, defer, traverse):
    on, off = _run(1, fold, defer, traverse), _reference()
    assert on.keys() == off.keys() == CASES.keys()
    for case in CASES:
        assert on[case].get("oracle") is True             # the worker compared this case with the oracle
        a, b = on[case]["values"], off[case]["values"]
        assert a.keys() == b.keys()
        assert len(a) == 3 + 2 * (CASES[case][1] - 2)     # lnl, persite, lnl2, every inner vector and scale buffer
        diff = [k for k in a if a[k] != b[k]]
        assert not diff, (case, diff[:8])


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("defer", [0, 3, 4])
def test_the_schedules_hold_every_kind_of_operation(product, defer, traverse):
    """pllhip_schedule_stats against the plan the host planner makes of the tree (the worker's TREE_SEEDS and PLANNED):
    a missing kind fails"""
    on, off = _run(1, 1, defer, traverse), _run(1, 0, defer, traverse)
    if common.FORCED:
        return                                # (how a list is scheduled is another matter under the forced modes)
    for case, (shape, ntips, _, rate_cats, coded, attrib, transient) in CASES.items():
        st = on[case]["stats"]
        assert 0 < st["chains"] < st["operations"], (case, st)              # some vector is handed over in registers
        if shape != "random" or not coded or attrib:
            continue
        if transient:
            assert st["folded_cherries"] >= 1 and st["lookup_children"] == 0, (case, st)     # (no class tables there)
            continue
        # the plan of the worker's comment: links with carried == 1 and == 2, folds under a first operation and under
        # links, inner vectors read from memory, a looked-up cherry x tip and (four rates) a looked-up cherry
        assert st == {"operations": ntips - 2, **PLANNED[rate_cats]}, (case, st)
        assert off[case]["stats"] == {"operations": ntips - 2, **PLANNED_NO_FOLDS[rate_cats]}, (case, off[case]["stats"])


def test_the_caterpillar_is_scaled_differently_from_site_to_site(product):
    """the vote, the handed-over counts and the counts of the fetch group at work: every site of the caterpillar is
    scaled, and not all the same"""
    res = _run(1, 1, 4, 1)
    ladders = [c for c in CASES if CASES[c][0] == "ladder"]
    assert len(ladders) == 4
    for case in ladders:
        assert res[case]["scaled_min"] > 0, (case, res[case]["scaled_min"])
        assert res[case]["scaled_max"] > res[case]["scaled_min"], case
    # (the counts themselves are compared bit for bit above)
