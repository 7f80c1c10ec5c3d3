"""Folded cherries (pll-modules_amd/csrc/kernels_s20.hpp, k_traverse_s20<..., FOLD>; pll_core.hip, plan_folds): the
20-state family builds a lone cherry -- a tip x tip operation that is a chain of its own -- in registers inside the
operation chain that reads it, instead of writing its vector and reading it back.  The cherry's vector and scaler
counts are still stored, and both paths execute the same floating-point operations in the same order, so everything a
caller can read must be EQUAL BIT FOR BIT to the same library planning without folds (PLLHIP_FOLD=0): every vector,
every scaler array, the likelihood and the per-site likelihoods, after full traversals, after partial lists that
read a folded cherry's vector from memory, from other root edges, and under evaluate-only traversals.  Any difference
is a bug, not rounding.  The folding run is compared with the CPU oracle as well, within the suite's tolerances.

PLLHIP_FOLD and PLLHIP_TRAVERSE (one launch per traversal / one per round of chains) are read once per process, so
each combination runs in a child process (tests/_fold_worker.py) that evaluates every case and writes digests."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import pytest

import common
from _fold_worker import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _run(fold, traverse):
    """the worker's results under PLLHIP_FOLD=fold, PLLHIP_TRAVERSE=traverse (the folding runs also check the oracle)"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "fold.json")
        env = {**os.environ, "PLLHIP_FOLD": str(fold), "PLLHIP_TRAVERSE": str(traverse)}
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fold_worker.py"), out, "1" if fold else "0"],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        with open(out) as f:
            return json.load(f)


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_folded_cherries_change_nothing_a_caller_can_see(product, case, traverse):
    on, off = _run(1, traverse)[case], _run(0, traverse)[case]
    assert on.get("oracle") is True                   # the worker compared this case with the oracle
    assert on["values"].keys() == off["values"].keys()
    diff = [k for k in on["values"] if on["values"][k] != off["values"][k]]
    assert not diff, f"not bit-identical to PLLHIP_FOLD=0: {diff[:8]} ({len(diff)} of {len(on['values'])})"


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_scheduler_reports_its_folds(product, case, traverse):
    on, off = _run(1, traverse)[case]["stats"], _run(0, traverse)[case]["stats"]
    shape, attrib = CASES[case][1], CASES[case][6]
    # (the statistics are those of the last resident schedule: the full traversal from the first root edge)
    assert off["folded_cherries"] == 0
    assert on["chains"] > 0 and off["chains"] > 0
    assert on["operations"] == off["operations"]
    assert on["inner_reads"] <= off["inner_reads"]
    if attrib or shape == "ladder" or common.FORCED_REPEATS:
        # per-rate scalers and site repeats plan as before; a ladder's one cherry is the bottom of the one chain
        assert on["folded_cherries"] == 0 and on == off
    else:
        assert on["folded_cherries"] >= 1
        # a fold saves a read unless it costs a cut; the plan as a whole never reads more
        assert on["inner_reads"] < off["inner_reads"]
        if shape == "balanced":
            # every second cherry is the lighter child of the node above it
            assert on["folded_cherries"] >= CASES[case][2] // 8
