"""Worker of test_lookup_children.py.  PLLHIP_LOOKUP, PLLHIP_LOOKUP_CLASSES and PLLHIP_TRAVERSE are read once per process, so
every combination runs in a process of its own: this one evaluates the cases named on its command line (default: all
of CASES) under the environment it was started with and writes one JSON file: per case the likelihoods, SHA-256
digests of every vector, scaler array and per-site likelihood a caller can read, and what pllhip_schedule_stats
reports.  argv: <output file> <oracle: 0 / 1> [case ...]; with oracle = 1 every case is also compared with the CPU
oracle within the suite's tolerances (an assertion failure ends the process with a non-zero status)."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import _fold_worker as fw

# name: (rate_cats, tree shape, ntips, nsites, gaps and ambiguity codes, scaled classes, attributes, transient)
# Light children (the smaller subtree under an operation with two inner children), counted on the CPU from
# pc.Tree(ntips, 42, 43) at its first root edge: random 24 taxa 3 cherries + 2 cherry x tip, random 40 taxa 4 + 1,
# random 60 taxa 9 + 1, random 120 taxa 15 + 6 (two of them ties), balanced 32 taxa 4 + 2.
CASES = {
    "random_r4": (4, "random", 24, 1031, False, False, "", False),
    "random_r2": (2, "random", 40, 2050, True, False, "", False),
    "random_r1": (1, "random", 60, 257, False, False, "", False),
    "deep_r4": (4, "random", 120, 700, False, False, "", False),
    "balanced_r4": (4, "balanced", 32, 4100, False, False, "", False),
    "scaled_r4": (4, "random", 24, 700, False, True, "", False),
    "rate_scalers_r4": fw.CASES["rate_scalers_r4"],
    "site_repeats_r4": fw.CASES["site_repeats_r4"],
    "transient_r4": fw.CASES["transient_r4"],
}


def make_tree(pc, shape, ntips, scaled):
    tree = pc.Tree(ntips, 42, 43, ladder=shape == "ladder", balanced=shape == "balanced")
    if scaled:
        # zero-length branches above two cherries out of three (as tests/_fold_worker.py has them) and above the tip of
        # every cherry x tip operation: a site whose two states differ is an all-zero, scaled column of such a cherry
        # and of the operation above it, so the looked-up classes carry scaling decisions, summed counts and zero rows
        is_cherry = {op[0]: op[2] < tree.ntips and op[5] < tree.ntips for op in tree.ops}
        ncherries = 0
        for op in tree.ops:
            kids = ((op[2], op[3]), (op[5], op[6]))
            if is_cherry[op[0]]:
                if ncherries % 3 != 2:
                    tree.brlens[op[3]] = 0.0
                    tree.brlens[op[6]] = 0.0 if ncherries % 3 == 0 else 0.05
                ncherries += 1
            else:
                for (c, m), (other, _) in (kids, kids[::-1]):
                    if c < tree.ntips and is_cherry.get(other, False):
                        tree.brlens[m] = 0.0
    return tree


def build(pc, lib, case, is_product):
    rate_cats, shape, ntips, nsites, gaps, scaled, attrib, transient = CASES[case]
    tree = make_tree(pc, shape, ntips, scaled)
    attributes = {"": 0, "rate_scalers": pc.PLL_ATTRIB_RATE_SCALERS, "site_repeats": pc.PLL_ATTRIB_SITE_REPEATS}[attrib]
    inst = pc.build_instance(lib, states=20, rate_cats=rate_cats, ntips=ntips, nsites=nsites, coded=True, tree=tree,
                             attributes=attributes)
    if gaps:
        # gaps and the ambiguity codes B / Z: 23 codes in use, 12 167 classes of three tips
        cmap = pc.state_charmap(20)
        cmap[ord("B")] = (1 << 2) | (1 << 3)
        cmap[ord("Z")] = (1 << 5) | (1 << 6)
        codes = pc.random_codes(ntips, nsites, 20, 44)
        rnd = pc.splitmix64(49, ntips * nsites).reshape(ntips, nsites)
        for t in range(ntips):
            seq = (codes[t] + 48).astype(np.uint8)
            seq[rnd[t] % np.uint64(17) == 0] = ord("-")
            seq[rnd[t] % np.uint64(23) == 1] = ord("B")
            seq[rnd[t] % np.uint64(29) == 2] = ord("Z")
            inst.set_tip_states(t, cmap, seq.tobytes())
    if transient and is_product:
        inst.set_transient(True)
    inst.tree = tree
    return inst, tree


def observe(pc, inst, tree, shape, scaled):
    """everything a caller can read, in the order a caller would: (name, array or number) pairs"""
    out = [("lnl", pc.full_traversal(inst))]
    stats = inst.schedule_stats() if inst.lib.is_product else None
    sa, sb = tree.scaler_of(tree.root_a), tree.scaler_of(tree.root_b)
    out.append(("persite", inst.edge_lnl(tree.root_a, sa, tree.root_b, sb, tree.root_matrix, persite=True)[1]))
    for op in tree.ops:
        out.append((f"clv{op[0]}", inst.get_clv(op[0])))
        out.append((f"scaler{op[1]}", inst.get_scaler(op[1])))
    # a second evaluation (the resident schedule is reused, its tables are built again)
    out.append(("lnl2", pc.full_traversal(inst)))
    # partial lists from two other root edges: the operations that differ read vectors and counts of looked-up
    # children from memory
    for k in (tree.nedges // 2, 1):
        t2 = make_tree(pc, shape, tree.ntips, scaled)
        t2.set_root_edge(k)
        old = {(o[0], frozenset((o[2], o[5]))) for o in tree.ops}
        part = [o for o in t2.ops_with_scalers(True) if (o[0], frozenset((o[2], o[5]))) not in old]
        inst.update_partials(part)
        for o in part:
            out.append((f"part{k}_clv{o[0]}", inst.get_clv(o[0])))
            out.append((f"part{k}_scaler{o[1]}", inst.get_scaler(o[1])))
        out.append((f"part{k}_lnl", inst.edge_lnl(t2.root_a, t2.scaler_of(t2.root_a), t2.root_b, t2.scaler_of(t2.root_b),
                                                  t2.root_matrix)))
        # ... then the whole tree from that edge, and back
        inst.tree = t2
        out.append((f"root{k}_lnl", pc.full_traversal(inst)))
        for op in t2.ops:
            out.append((f"root{k}_clv{op[0]}", inst.get_clv(op[0])))
            out.append((f"root{k}_scaler{op[1]}", inst.get_scaler(op[1])))
        inst.tree = tree
        out.append((f"back{k}_lnl", pc.full_traversal(inst)))
    return out, stats


def main():
    out_file, with_oracle = sys.argv[1], sys.argv[2] == "1"
    cases = sys.argv[3:] or list(CASES)
    import pllhip_ctypes as pc
    from test_gpu_parity import lnl_close, site_err, REL_CLV
    product = pc.PllLib(pc.PRODUCT_LIB)
    oracle = pc.PllLib(os.environ.get("PLLHIP_ORACLE_LIB") or os.path.join(ROOT, "oracle", "_build", "libpll_oracle.so")) \
        if with_oracle else None
    result = {}
    for case in cases:
        spec = CASES[case]
        inst, tree = build(pc, product, case, True)
        with inst:
            got, stats = observe(pc, inst, tree, spec[1], spec[5])
        entry = {"stats": {"chains": stats.chains, "operations": stats.operations, "inner_reads": stats.inner_reads,
                           "folded_cherries": stats.folded_cherries, "lookup_children": stats.lookup_children},
                 "values": {}}
        for name, v in got:
            if isinstance(v, np.ndarray):
                entry["values"][name] = hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
            else:
                entry["values"][name] = float(v).hex()
        result[case] = entry
        if oracle is not None:
            ref_inst, ref_tree = build(pc, oracle, case, False)
            with ref_inst:
                ref, _ = observe(pc, ref_inst, ref_tree, spec[1], spec[5])
            assert [n for n, _ in got] == [n for n, _ in ref], case
            nsites = spec[3]
            for (name, a), (_, b) in zip(got, ref):
                if "scaler" in name:
                    assert np.array_equal(a, b), (case, name)                       # integers: exact
                elif "clv" in name:
                    assert site_err(np.asarray(a), np.asarray(b)) <= REL_CLV, (case, name)
                elif name == "persite":
                    fin = np.isfinite(b)
                    assert np.array_equal(fin, np.isfinite(a)), (case, name)
                    assert np.all(np.abs(a[fin] - b[fin]) <= 1e-10 * np.abs(b[fin]) + 1e-11), (case, name)
                elif np.isfinite(b):
                    assert lnl_close(a, b, nsites, 20), (case, name, a, b)
                else:
                    assert a == b, (case, name, a, b)
            entry["oracle"] = True
    with open(out_file, "w") as f:
        json.dump(result, f)


if __name__ == "__main__":
    main()
