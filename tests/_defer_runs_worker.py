"""Worker of test_deferred_runs.py.  PLLHIP_DEFER, PLLHIP_DEFER_DEPTH, PLLHIP_DEFER_GROUP, PLLHIP_LOOKUP and
PLLHIP_TRAVERSE are read once per process, so every combination runs in a process of its own.  This one takes every
case of _defer_worker.CASES through the checkpoints of _defer_worker.observe and through two more that aim at the
deferred runs at the bottom of chains (plan_defers, level 3):

  probe    -- per caterpillar of the tree (a cherry of tips and the "x tip" operations above it), after a fresh full
              traversal: the vectors are read bottom-up, one reader at a time, and what each reader stored later is
              recorded (the group store brings a whole run along with its bottom cherry);
  partial  -- per caterpillar of two and more operations (the two longest): the list that re-roots the tree towards
              the pendant edge of the tip of its second (and third) operation -- it reads the members below from
              memory and overwrites the ones above --, with the counters before and after.

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

from _defer_worker import CASES, bench_pattern, digest, make_tree, observe, partial_list, readable


def caterpillars(tree):
    """[[cherry, the operation above it, ...]] (node indices, bottom-up): a cherry of tips and, as long as they go,
    the operations that join the node below with a tip"""
    by_parent = {op[0]: op for op in tree.ops}
    consumer = {}
    for op in tree.ops:
        consumer[op[2]] = consumer[op[5]] = op
    out = []
    for op in tree.ops:
        if op[2] >= tree.ntips or op[5] >= tree.ntips:
            continue
        run = [op[0]]
        while run[-1] in consumer:
            up = consumer[run[-1]]
            other = up[5] if up[2] == run[-1] else up[2]
            if other >= tree.ntips:
                break
            run.append(up[0])
        out.append(run)
    assert all(n in by_parent for run in out for n in run)
    return out


def tip_of(tree, node, below):
    """the tip child of `node`, whose other child is `below`"""
    op = {o[0]: o for o in tree.ops}[node]
    return op[5] if op[2] == below else op[2]


def pendant_edge(tree, node, tip):
    op = {o[0]: o for o in tree.ops}[node]
    return op[3] if op[2] == tip else op[6]


def observe_runs(pc, inst, tree, shape):
    """the two checkpoints of the module's docstring: (name, value) pairs and the counters (product library only)"""
    is_product = inst.lib.is_product
    out, probes, partials = [], [], []

    def deferred():
        if not is_product:
            return [0, 0, 0]
        st = inst.deferred_stats()
        return [st.deferred, st.stored_later, st.given_up]

    runs = caterpillars(tree)
    pc.full_traversal(inst)
    for run in runs:
        stored = []
        for n in run:
            before = deferred()[1]
            out.append((f"probe{run[0]}_clv{n}", inst.get_clv(n)))
            stored.append(deferred()[1] - before)
        probes.append({"nodes": run, "stored_later": stored})
    out.append(("probe_lnl", pc.full_traversal(inst)))

    for run in sorted((r for r in runs if len(r) >= 2), key=lambda r: (-len(r), r[0]))[:2]:
        for j in (1, 2):
            if j >= len(run):
                continue
            tip = tip_of(tree, run[j], run[j - 1])
            pc.full_traversal(inst)
            t2, part = partial_list(pc, tree, shape, pendant_edge(tree, run[j], tip))
            if not part:                                # (the tree is rooted there already)
                continue
            before = deferred()
            inst.update_partials(part)
            after = deferred()
            tag = f"above{run[0]}_{j}"
            sa, sb = t2.scaler_of(t2.root_a), t2.scaler_of(t2.root_b)
            out.append((f"{tag}_lnl", inst.edge_lnl(t2.root_a, sa, t2.root_b, sb, t2.root_matrix)))
            out += readable(inst, t2, tag, part)
            out += readable(inst, tree, f"{tag}_old", [o for o in tree.ops if o[0] not in {p[0] for p in part}])
            partials.append({"nodes": run, "member": j, "before": before, "after": after, "end": deferred(),
                             "written": [p[0] for p in part],
                             "read": [c for p in part for c in (p[2], p[5]) if c not in {q[0] for q in part}]})
    return out, {"probes": probes, "partials": partials}


def compare(case, nsites, got, ref):
    from test_gpu_parity import lnl_close, site_err, REL_CLV
    ref = dict(ref)
    for name, a in got:
        if name.startswith("anc_"):
            continue                                                     # (the product's own call)
        b = ref[name]
        if "scaler" in name:
            assert np.array_equal(a, b), (case, name)                       # integers: exact
        elif "clv" in name:
            assert site_err(np.asarray(a), np.asarray(b)) <= REL_CLV, (case, name)
        elif name.endswith("persite"):
            fin = np.isfinite(b)
            assert np.array_equal(fin, np.isfinite(a)), (case, name)
            assert np.all(np.abs(a[fin] - b[fin]) <= 1e-10 * np.abs(b[fin]) + 1e-11), (case, name)
        elif name.endswith("deriv"):
            assert np.allclose(a, b, rtol=1e-8), (case, name, a, b)
        elif np.isfinite(b):
            assert lnl_close(a, b, nsites, 20), (case, name, a, b)
        else:
            assert a == b, (case, name, a, b)


ADAPTIVE = (24, 123_008)        # taxa, sites: 3 844 site blocks, just above the floor of deferred stores (3 840)


def adaptive(pc, lib):
    """without PLLHIP_DEFER the level follows the caller: four full traversals in a row, every vector read, three more
    traversals -- the counters after each, the likelihoods, and digests of what was read"""
    ntips, nsites = ADAPTIVE
    tree = pc.Tree(ntips, 42, 43)
    inst = pc.build_instance(lib, states=20, rate_cats=4, ntips=ntips, nsites=nsites, coded=True, tree=tree)
    stats, lnl = [], []

    def step():
        lnl.append(float(pc.full_traversal(inst)).hex())
        st = inst.deferred_stats()
        stats.append([st.deferred, st.stored_later, st.given_up])

    with inst:
        for _ in range(4):
            step()
        read = [digest(inst.get_clv(op[0])) for op in tree.ops]
        for _ in range(3):
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
            counters["runs"] = runs
            return got + more, counters
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
