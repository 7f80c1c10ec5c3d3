"""Worker of test_deferred_chains.py.  PLLHIP_DEFER, PLLHIP_DEFER_GROUP, PLLHIP_LOOKUP and PLLHIP_TRAVERSE are read once
per process, so every combination runs in a process of its own.  This one takes every case of _defer_worker.CASES
through the checkpoints of _defer_worker.observe and _defer_runs_worker.observe_runs and through one more that aims at
the vectors level 4 of plan_defers leaves out inside the chains -- vectors that are recomputed from stored child
vectors and P-matrices, not from tip codes alone:

  pmat     -- per inner node below the root edge with an inner child, after a fresh full traversal: the P-matrix of the
              branch to that child gets another length and the likelihood at the root edge is asked for (which makes the
              matrix change on the device); then the node's vector is read.  It must be the vector of the traversal, made
              with the old matrix, so the engine has to store it before the matrix changes: the counters are recorded
              before the change, after it and after the read.

argv: <output file> <oracle: 0 / 1> [adaptive]; "adaptive": the checkpoint of `adaptive` alone (a partition at the size
floor of deferred stores, for the runs that leave PLLHIP_DEFER unset).  With oracle = 1 every value is also compared
with the CPU oracle within the suite's tolerances (an assertion failure ends the process with a non-zero status)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

from _defer_worker import CASES, bench_pattern, digest, make_tree, observe, root_lnl
from _defer_runs_worker import ADAPTIVE, compare, observe_runs

# S20_DEFER_CHAIN_ROW of pll_core.hip: the lists in a row that must have gone unread before the default plans level 4
CHAIN_ROW = 4


def inner_sided(tree):
    """[(node, the P-matrix of the branch to an inner child of it)] for the operations with an inner child whose vector
    an operation of the list reads (not the two ends of the root edge), in post-order"""
    read = {c for op in tree.ops for c in (op[2], op[5])}
    return [(op[0], op[3] if op[2] >= tree.ntips else op[6]) for op in tree.ops
            if op[0] in read and (op[2] >= tree.ntips or op[5] >= tree.ntips)]


def observe_pmat(pc, inst, tree):
    """the checkpoint of the module's docstring: (name, value) pairs and the counters (product library only)"""
    is_product = inst.lib.is_product
    out, records = [], []

    def deferred():
        if not is_product:
            return [0, 0, 0]
        st = inst.deferred_stats()
        return [st.deferred, st.stored_later, st.given_up]

    for node, m in inner_sided(tree):
        pc.full_traversal(inst)
        before = deferred()
        inst.update_pmatrices([m], [tree.brlens[m] * 2.3])
        out.append((f"pmat{node}_lnl", root_lnl(inst, tree)))
        changed = deferred()
        out.append((f"pmat{node}_clv{node}", inst.get_clv(node)))
        records.append({"node": node, "matrix": int(m), "before": before, "changed": changed, "read": deferred()})
        inst.update_pmatrices([m], [tree.brlens[m]])
    out.append(("pmat_lnl", pc.full_traversal(inst)))
    return out, records


def adaptive(pc, lib):
    """without PLLHIP_DEFER the level follows the caller: CHAIN_ROW + 2 full traversals in a row, every vector read,
    CHAIN_ROW + 2 more -- the counters after each, the likelihoods, and digests of what was read"""
    ntips, nsites = ADAPTIVE
    tree = pc.Tree(ntips, 42, 43)
    inst = pc.build_instance(lib, states=20, rate_cats=4, ntips=ntips, nsites=nsites, coded=True, tree=tree)
    stats, lnl = [], []

    def step():
        lnl.append(float(pc.full_traversal(inst)).hex())
        st = inst.deferred_stats()
        stats.append([st.deferred, st.stored_later, st.given_up])

    with inst:
        for _ in range(CHAIN_ROW + 2):
            step()
        read = [digest(inst.get_clv(op[0])) for op in tree.ops]
        for _ in range(CHAIN_ROW + 2):
            step()
    return {"lnl": lnl, "deferred": stats, "read": read}


def main():
    out_file, with_oracle = sys.argv[1], sys.argv[2] == "1"
    import pllhip_ctypes as pc
    product = pc.PllLib(pc.PRODUCT_LIB)
    if len(sys.argv) > 3 and sys.argv[3] == "adaptive":
        with open(out_file, "w") as f:
            json.dump({"adaptive": adaptive(pc, product)}, f)
        return
    oracle = pc.PllLib(os.environ.get("PLLHIP_ORACLE_LIB") or os.path.join(ROOT, "oracle", "_build", "libpll_oracle.so")) \
        if with_oracle else None
    result = {}
    for case, (shape, ntips, nsites) in CASES.items():
        def both(lib):
            tree = make_tree(pc, shape, ntips)
            inst = pc.build_instance(lib, states=20, rate_cats=4, ntips=ntips, nsites=nsites, coded=True, tree=tree)
            with inst:
                got, counters = observe(pc, inst, tree, shape, nsites)
                more, runs = observe_runs(pc, inst, tree, shape)
                pmat, records = observe_pmat(pc, inst, tree)
            counters["runs"] = runs
            counters["pmat"] = records
            return got + more + pmat, counters
        got, counters = both(product)
        entry = {"counters": counters, "values": {name: digest(v) for name, v in got}}
        assert len(entry["values"]) == len(got)                              # (no name twice)
        result[case] = entry
        if oracle is not None:
            compare(case, nsites, got, both(oracle)[0])
            entry["oracle"] = True
    result["bench"] = bench_pattern(pc, product)
    with open(out_file, "w") as f:
        json.dump(result, f)


if __name__ == "__main__":
    main()
