"""Worker of test_chain_op_order.py.  PLLHIP_CHAINS, PLLHIP_LOOKUP, PLLHIP_FOLD, PLLHIP_DEFER and PLLHIP_TRAVERSE are read
once per process, so every combination runs in a process of its own: this one evaluates every case of CASES under the
environment it was started with and writes one JSON file: per case the likelihood, digests of every inner vector, every
scale buffer and the per-site likelihoods, the summed scaler counts per site and what pllhip_schedule_stats reports.
argv: <output file> <oracle: 0 / 1>; with oracle = 1 every case is also compared with the CPU oracle within the
tolerances of tests/test_gpu_parity.py (an assertion failure ends the process with a non-zero status)."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

# The 24-taxon random tree.  Its seeds were picked with the host planner (csrc/chain_plan.cpp, driven as
# tests/chain_plan_host_check.cpp drives it, with the 20-state family's limits: chains of at most 8 operations, 20 480
# doubles of LDS, 20 codes in use) so that one schedule holds every kind of operation s20_chain_op knows.  With four
# rates, folds and class tables it plans 6 chains over the 22 operations: 7 links with carried == 1, 6 with
# carried == 2, 3 folded cherries (one under the first operation of a chain, two under links), 2 class-table children
# (one cherry, one cherry x tip, both under links) and 3 inner vectors read from memory.  With one or two rates the
# tables are smaller and the chains longer: 4 chains, 8 + 6 links, 4 folds, one class-table child (cherry x tip).
# Without folds: 9 chains, 8 + 5 links, 8 inner reads (four rates); 8 chains, 8 + 6 links, 7 inner reads (one, two).
TREE_SEEDS = (2, 3)
# rates -> what pllhip_schedule_stats must report of the plain coded storing traversal
PLANNED = {4: {"chains": 6, "folded_cherries": 3, "lookup_children": 2, "inner_reads": 3},
           2: {"chains": 4, "folded_cherries": 4, "lookup_children": 1, "inner_reads": 2},
           1: {"chains": 4, "folded_cherries": 4, "lookup_children": 1, "inner_reads": 2}}
PLANNED_NO_FOLDS = {4: {"chains": 9, "folded_cherries": 0, "lookup_children": 0, "inner_reads": 8},       # PLLHIP_FOLD=0
                    2: {"chains": 8, "folded_cherries": 0, "lookup_children": 0, "inner_reads": 7},
                    1: {"chains": 8, "folded_cherries": 0, "lookup_children": 0, "inner_reads": 7}}


def cases():
    """name: (tree, ntips, nsites, rate_cats, coded tips, attribute, evaluate-only)"""
    out = {}
    for nsites in (95, 33):                       # three site blocks, the last one partial; two
        for rate_cats in (1, 2, 4):
            for coded, attrib in ((True, ""), (True, "rate_scalers"), (True, "site_repeats"), (False, "")):
                for transient in (False, True):
                    name = f"random_n{nsites}_r{rate_cats}_{'coded' if coded else 'vector'}_{attrib or 'plain'}" \
                           f"{'_evaluate' if transient else ''}"
                    out[name] = ("random", 24, nsites, rate_cats, coded, attrib, transient)
    # a caterpillar with long branches: every vector near the top is scaled, sites differ in how often
    for attrib in ("", "rate_scalers"):
        for transient in (False, True):
            out[f"ladder_r4_{attrib or 'plain'}{'_evaluate' if transient else ''}"] = ("ladder", 64, 95, 4, True, attrib, transient)
    return out


CASES = cases()


def make_tree(pc, shape, ntips):
    if shape == "ladder":
        return pc.Tree(ntips, 42, 43, brlen_range=(1.0, 2.5), ladder=True)
    return pc.Tree(ntips, *TREE_SEEDS)


def build(pc, lib, case, is_product):
    shape, ntips, nsites, rate_cats, coded, attrib, transient = CASES[case]
    tree = make_tree(pc, shape, ntips)
    attributes = {"": 0, "rate_scalers": pc.PLL_ATTRIB_RATE_SCALERS, "site_repeats": pc.PLL_ATTRIB_SITE_REPEATS}[attrib]
    inst = pc.build_instance(lib, states=20, rate_cats=rate_cats, ntips=ntips, nsites=nsites, coded=coded, tree=tree,
                             attributes=attributes)
    # (coded = False: without PLL_ATTRIB_PATTERN_TIP every tip is a vector in memory, read like an inner vector)
    if transient and is_product:
        inst.set_transient(True)
    inst.tree = tree
    return inst, tree


def observe(pc, inst, tree):
    """everything a caller can read, in the order a caller would: (name, array or number) pairs"""
    out = [("lnl", pc.full_traversal(inst))]
    stats = inst.schedule_stats() if inst.lib.is_product else None
    sa, sb = tree.scaler_of(tree.root_a), tree.scaler_of(tree.root_b)
    out.append(("persite", inst.edge_lnl(tree.root_a, sa, tree.root_b, sb, tree.root_matrix, persite=True)[1]))
    for op in tree.ops:
        out.append((f"clv{op[0]}", inst.get_clv(op[0])))
        out.append((f"scaler{op[1]}", inst.get_scaler(op[1])))
    # a second evaluation (the resident schedule is reused)
    out.append(("lnl2", pc.full_traversal(inst)))
    return out, stats


def scaled_sites(inst, tree, got):
    """scaler counts summed per site over every scale buffer (and over the rates with per-rate scalers): counts add up
    towards the root, so the sum tells how early a site was scaled first as well as how often"""
    values = dict(got)
    total = np.zeros(inst.N, dtype=np.int64)
    for op in tree.ops:
        total += values[f"scaler{op[1]}"].astype(np.int64).reshape(inst.N, -1).sum(axis=1)
    return total


def main():
    out_file, with_oracle = sys.argv[1], sys.argv[2] == "1"
    import pllhip_ctypes as pc
    from test_gpu_parity import lnl_close, site_err, REL_CLV
    product = pc.PllLib(pc.PRODUCT_LIB)
    oracle = pc.PllLib(os.environ.get("PLLHIP_ORACLE_LIB") or os.path.join(ROOT, "oracle", "_build", "libpll_oracle.so")) \
        if with_oracle else None
    result = {}
    for case, spec in CASES.items():
        inst, tree = build(pc, product, case, True)
        with inst:
            got, stats = observe(pc, inst, tree)
            counts = scaled_sites(inst, tree, got)
        entry = {"stats": {"chains": stats.chains, "operations": stats.operations, "inner_reads": stats.inner_reads,
                           "folded_cherries": stats.folded_cherries, "lookup_children": stats.lookup_children},
                 "scaled_min": int(counts.min()), "scaled_max": int(counts.max()), "values": {}}
        for name, v in got:
            if isinstance(v, np.ndarray):
                entry["values"][name] = hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
            else:
                entry["values"][name] = float(v).hex()
        assert len(entry["values"]) == len(got)                              # (no name twice)
        result[case] = entry
        if oracle is not None:
            ref_inst, ref_tree = build(pc, oracle, case, False)
            with ref_inst:
                ref, _ = observe(pc, ref_inst, ref_tree)
            assert [n for n, _ in got] == [n for n, _ in ref], case
            for (name, a), (_, b) in zip(got, ref):
                if "scaler" in name:
                    assert np.array_equal(a, b), (case, name)                       # integers: exact
                elif "clv" in name:
                    assert site_err(np.asarray(a), np.asarray(b)) <= REL_CLV, (case, name)
                elif name == "persite":
                    fin = np.isfinite(b)
                    assert np.array_equal(fin, np.isfinite(a)), (case, name)
                    assert np.all(np.abs(a[fin] - b[fin]) <= 1e-10 * np.abs(b[fin]) + 1e-11), (case, name)
                else:
                    assert np.isfinite(b) and lnl_close(a, b, spec[2], 20), (case, name, a, b)
            entry["oracle"] = True
    with open(out_file, "w") as f:
        json.dump(result, f)


if __name__ == "__main__":
    main()
