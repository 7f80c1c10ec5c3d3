"""Small light subtrees read from class tables (pll-modules_amd/csrc/kernels_s20.hpp, k_traverse_s20<..., LOOK>;
pll_core.hip, plan_lookups / emit_lookup_tables): where a 20-state operation chain meets a lone cherry that was not
folded, or a cherry x tip operation, as its light child, the consumer gathers rows of a table over all classes of tip
codes instead of reading the child's vector back.  The child's chain still stores vector and scaler counts, the rows
are made by the class kernels whose consumers site repeats pins to the per-site result, so everything a caller can
read must be EQUAL BIT FOR BIT to the same library planning without such reads (PLLHIP_LOOKUP=0): every vector, every
scaler array, the likelihood and the per-site likelihoods, after full traversals, after partial lists that read a
looked-up child's vector from memory, and from other root edges.  Any difference is a bug, not rounding.  The run with
the reads is compared with the CPU oracle as well, within the suite's tolerances.

PLLHIP_LOOKUP (1: such reads at any partition size -- by default they start at 8192 site blocks --, 0: none),
PLLHIP_LOOKUP_CLASSES and PLLHIP_TRAVERSE (one launch per traversal / one per round of chains) are read once per process, so each combination runs in a child process (tests/_lookup_worker.py) that evaluates every case and
writes digests."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import pytest

import common
from _lookup_worker import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the committed class limit of plan_lookups admits cherry x tip children (U^3 classes), not cherries alone
DEFAULT_ADMITS_TRIPLES = True


@functools.lru_cache(maxsize=None)
def _run(lookup, traverse, classes=None, cases=()):
    """the worker's results under PLLHIP_LOOKUP=lookup, PLLHIP_TRAVERSE=traverse (the runs with the reads also check
    the oracle)"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "lookup.json")
        env = {**os.environ, "PLLHIP_LOOKUP": str(lookup), "PLLHIP_TRAVERSE": str(traverse)}
        env.pop("PLLHIP_LOOKUP_CLASSES", None)
        if classes is not None:
            env["PLLHIP_LOOKUP_CLASSES"] = str(classes)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_lookup_worker.py"), out, "1" if lookup else "0", *cases],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        with open(out) as f:
            return json.load(f)


def _same_values(on, off, what):
    assert on["values"].keys() == off["values"].keys()
    diff = [k for k in on["values"] if on["values"][k] != off["values"][k]]
    assert not diff, f"not bit-identical to {what}: {diff[:8]} ({len(diff)} of {len(on['values'])})"


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_class_table_reads_change_nothing_a_caller_can_see(product, case, traverse):
    on, off = _run(1, traverse)[case], _run(0, traverse)[case]
    assert on.get("oracle") is True                   # the worker compared this case with the oracle
    _same_values(on, off, "PLLHIP_LOOKUP=0")


@pytest.mark.parametrize("traverse", [1, 0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_scheduler_reports_its_lookups(product, case, traverse):
    on, off = _run(1, traverse)[case]["stats"], _run(0, traverse)[case]["stats"]
    attrib, transient = CASES[case][6], CASES[case][7]
    # (the statistics are those of the last resident schedule: the full traversal from the first root edge)
    assert off["lookup_children"] == 0
    assert on["chains"] > 0 and off["chains"] > 0
    for name in ("operations", "chains", "folded_cherries"):
        assert on[name] == off[name], name
    assert on["inner_reads"] == off["inner_reads"] - on["lookup_children"]
    if attrib or transient or common.FORCED:
        # per-rate scalers, site repeats and evaluate-only traversals (also when the suite forces them) plan as before
        assert on == off
    elif case in ("random_r4", "deep_r4") and DEFAULT_ADMITS_TRIPLES:
        assert on["lookup_children"] >= 2               # their cherry x tip children
    elif case in ("random_r4", "deep_r4") and on["folded_cherries"] < (3 if case == "random_r4" else 15):
        assert on["lookup_children"] >= 1               # a light cherry (3 / 15 of them) that was not folded


def test_a_class_limit_of_pairs_plans_cherries_only(product):
    """23 codes in use: PLLHIP_LOOKUP_CLASSES=529 admits the 529 classes of a cherry and not the 12 167 of three tips"""
    few = _run(1, 1, 529, ("random_r2",))["random_r2"]
    on, off = _run(1, 1)["random_r2"], _run(0, 1)["random_r2"]
    assert few.get("oracle") is True
    _same_values(few, off, "PLLHIP_LOOKUP=0")
    assert few["stats"]["inner_reads"] == off["stats"]["inner_reads"] - few["stats"]["lookup_children"]
    if not common.FORCED:
        assert few["stats"]["lookup_children"] <= on["stats"]["lookup_children"]
        if DEFAULT_ADMITS_TRIPLES:
            # random, 40 taxa: one cherry x tip light child next to four light cherries
            assert few["stats"]["lookup_children"] < on["stats"]["lookup_children"]
