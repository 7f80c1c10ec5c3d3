"""Worker of test_deferred_stores.py.  PLLHIP_DEFER, PLLHIP_LOOKUP and PLLHIP_TRAVERSE are read once per process, so
every combination runs in a process of its own: this one takes every case of CASES through the checkpoints of
`observe` under the environment it was started with and writes one JSON file: per case the digests of everything a
caller can read at every checkpoint, what pllhip_schedule_stats / pllhip_deferred_stats / pllhip_transient_stats
report, and the benchmark's pattern (BENCH) on the side.  argv: <output file> <oracle: 0 / 1>; with oracle = 1 every
case is also compared with the CPU oracle within the suite's tolerances (an assertion failure ends the process with
a non-zero status)."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

# name: (tree shape, ntips, nsites); 20 states, four rates.  1 031 and 4 100 sites: no multiple of the 32-site block,
# the last block partial, one and several blocks per wave
CASES = {
    "random14_1031": ("random", 14, 1031),
    "random14_4100": ("random", 14, 4100),
    "random40_4100": ("random", 40, 4100),
    "random60_1031": ("random", 60, 1031),
    "balanced32_1031": ("balanced", 32, 1031),
    "balanced32_4100": ("balanced", 32, 4100),
    "ladder20_1031": ("ladder", 20, 1031),
}
BENCH = (24, 1031)              # taxa, sites of the benchmark's pattern


def make_tree(pc, shape, ntips):
    return pc.Tree(ntips, 42, 43, ladder=shape == "ladder", balanced=shape == "balanced")


def light_cherries(tree):
    """(cherry, its consumer, the matrix between them, the matrix between the consumer and its other child) for the
    cherries that sit next to an inner sibling: the ones a chain can meet as its light child"""
    by_parent = {op[0]: op for op in tree.ops}
    out = []
    for op in tree.ops:
        for x, y in ((2, 5), (5, 2)):
            c = by_parent.get(op[x])
            if c is not None and c[2] < tree.ntips and c[5] < tree.ntips and op[y] >= tree.ntips:
                out.append((c[0], op[0], op[x + 1], op[y + 1]))
    return out


def partial_list(pc, tree, shape, k):
    """the operations of the orientation towards edge k that differ from the tree's: what a partial traversal issues"""
    t2 = make_tree(pc, shape, tree.ntips)
    t2.set_root_edge(k)
    old = {(o[0], frozenset((o[2], o[5]))) for o in tree.ops}
    return t2, [o for o in t2.ops if (o[0], frozenset((o[2], o[5]))) not in old]


def readable(inst, tree, tag, ops=None):
    """every vector and scaler array of `ops` (default: the tree's), in post-order"""
    out = []
    for op in (tree.ops if ops is None else ops):
        out.append((f"{tag}_clv{op[0]}", inst.get_clv(op[0])))
        out.append((f"{tag}_scaler{op[1]}", inst.get_scaler(op[1])))
    return out


def root_lnl(inst, tree, persite=False):
    return inst.edge_lnl(tree.root_a, tree.scaler_of(tree.root_a), tree.root_b, tree.scaler_of(tree.root_b),
                         tree.root_matrix, persite=persite)


def observe(pc, inst, tree, shape, nsites):
    """the checkpoints, each from a fresh full traversal (which defers again): (name, array or number) pairs, and the
    counters (product library only)"""
    is_product = inst.lib.is_product
    out, counters = [], {}

    def deferred():
        st = inst.deferred_stats()
        return [st.deferred, st.stored_later, st.given_up]

    # after a full traversal: the likelihoods, then every vector, one reader at a time
    out.append(("full_lnl", pc.full_traversal(inst)))
    if is_product:
        st = inst.schedule_stats()
        counters["schedule"] = {n: getattr(st, n) for n in ("chains", "operations", "inner_reads", "folded_cherries", "lookup_children")}
        counters["after_first"] = deferred()
    out.append(("full_persite", root_lnl(inst, tree, True)[1]))
    per_reader = []
    for op in tree.ops:
        before = deferred()[1] if is_product else 0
        out.append((f"full_clv{op[0]}", inst.get_clv(op[0])))
        per_reader.append((deferred()[1] if is_product else 0) - before)
        out.append((f"full_scaler{op[1]}", inst.get_scaler(op[1])))
    if is_product:
        counters["per_reader"] = per_reader
        counters["after_readers"] = deferred()
    out.append(("full_lnl2", pc.full_traversal(inst)))

    # new lengths on every branch: the vectors are the old ones
    pc.full_traversal(inst)
    inst.update_pmatrices(np.arange(tree.nedges), tree.brlens * 1.7)
    out += readable(inst, tree, "brlen")
    out.append(("brlen_lnl", root_lnl(inst, tree)))

    # a changed tip (and back)
    cmap = pc.state_charmap(20)
    codes = pc.random_codes(tree.ntips, nsites, 20, 44)
    by_parent = {op[0]: op for op in tree.ops}
    tip = by_parent[light_cherries(tree)[0][0]][2] if light_cherries(tree) else 3      # a tip of a light cherry
    pc.full_traversal(inst)
    inst.set_tip_states(tip, cmap, (pc.random_codes(tree.ntips, nsites, 20, 77)[tip] + 48).tobytes())
    out += readable(inst, tree, "tip")
    out.append(("tip_lnl", pc.full_traversal(inst)))
    inst.set_tip_states(tip, cmap, (codes[tip] + 48).tobytes())

    # partial lists from other root edges: towards the edge above a light cherry (the cherry is read from memory by the
    # edge likelihood, the sumtable and the derivatives), towards the edge between its consumer and the consumer's other
    # child (the consumer's new operation reads the cherry from memory), towards the pendant edge of one of its tips (the
    # cherry's vector and scaler buffer are overwritten), and two edges elsewhere
    edges = [tree.nedges // 2, 1]
    for c, _, m, m_other in light_cherries(tree)[:2]:
        edges += [m, m_other, by_parent[c][3]]
    reads = overwrites = 0
    for k in sorted(set(edges)):
        pc.full_traversal(inst)
        t2, part = partial_list(pc, tree, shape, k)
        before = deferred() if is_product else None
        inst.update_partials(part)
        if is_product:
            after = deferred()
            reads += after[1] - before[1]
            overwrites += after[2] - before[2]
        sa, sb = t2.scaler_of(t2.root_a), t2.scaler_of(t2.root_b)
        out.append((f"part{k}_lnl", inst.edge_lnl(t2.root_a, sa, t2.root_b, sb, t2.root_matrix)))
        st = inst.alloc_sumtable()
        inst.update_sumtable(t2.root_a, t2.root_b, sa, sb, st)
        out.append((f"part{k}_deriv", np.asarray([inst.derivatives(sa, sb, x, st) for x in (0.01, 0.3)])))
        inst.free_sumtable(st)
        out += readable(inst, t2, f"part{k}", part)
        out += readable(inst, tree, f"part{k}_old", [o for o in tree.ops if o[0] not in {p[0] for p in part}])
    if is_product:
        counters["partial_reads"], counters["partial_overwrites"] = reads, overwrites

    # a sumtable and derivatives alone, on the edge above a light cherry, straight after the partial list
    for c, _, m, _ in light_cherries(tree)[:1]:
        pc.full_traversal(inst)
        t2, part = partial_list(pc, tree, shape, m)
        inst.update_partials(part)
        sa, sb = t2.scaler_of(t2.root_a), t2.scaler_of(t2.root_b)
        st = inst.alloc_sumtable()
        inst.update_sumtable(t2.root_a, t2.root_b, sa, sb, st)
        out.append(("sum_deriv", np.asarray([inst.derivatives(sa, sb, x, st) for x in (0.02, 0.5)])))
        inst.free_sumtable(st)

    # marginal ancestral states over all nodes (the product's own call)
    pc.full_traversal(inst)
    if is_product:
        triples = [(op[0], op[2], op[3]) for op in tree.ops] + [(op[0], op[5], op[6]) for op in tree.ops]
        states, probs, _ = inst.node_ancestral_batch(*zip(*triples))
        out.append(("anc_states", states))
        out.append(("anc_probs", probs))
    out += readable(inst, tree, "anc")

    # host mirror and back
    pc.full_traversal(inst)
    if is_product:
        assert inst.L.pllhip_sync_to_host(inst.p, pc.PLLHIP_SYNC_ALL)
        assert inst.L.pllhip_sync_to_device(inst.p, pc.PLLHIP_SYNC_ALL)
    out += readable(inst, tree, "sync")
    out.append(("sync_lnl", root_lnl(inst, tree)))

    # evaluate-only traversals switched on after a deferring traversal, and off again
    pc.full_traversal(inst)
    if is_product:
        inst.set_transient(True)
    out.append(("mode_on_lnl", pc.full_traversal(inst)))
    out += readable(inst, tree, "mode_on")
    if is_product:
        inst.set_transient(False)
    out.append(("mode_off_lnl", pc.full_traversal(inst)))
    out += readable(inst, tree, "mode_off")

    # pllhip_discard_transient: nothing of a storing traversal is the caller's to give up
    pc.full_traversal(inst)
    if is_product:
        inst.discard_transient()
    out += readable(inst, tree, "discard")
    out.append(("discard_lnl", root_lnl(inst, tree)))
    if is_product:
        ts = inst.transient_stats()
        counters["transient"] = [ts.skipped, ts.materialized, ts.discarded]
    return out, counters


def bench_pattern(pc, lib):
    """the benchmark's step at small size: the driver's full evaluation (per-branch P-matrix calls, the whole tree, the
    likelihood at the root), four in a row"""
    ntips, nsites = BENCH
    tree = pc.Tree(ntips, 42, 43)
    codes = pc.random_codes(ntips, nsites, 20, 44)
    subst, freqs = pc.protein_model()
    with pc.Evaluation(lib, tree.newick()) as ev:
        inst = ev.add_partition(0, 20, nsites, 4, codes, subst, freqs, 0.7)
        lnl, stats = [], []
        for _ in range(4):
            lnl.append(float(ev.loglh()).hex())
            st = inst.deferred_stats()
            stats.append([st.deferred, st.stored_later, st.given_up])
        ts = inst.transient_stats()
    return {"lnl": lnl, "deferred": stats, "transient": [ts.skipped, ts.materialized, ts.discarded]}


def digest(v):
    if isinstance(v, np.ndarray):
        return hashlib.blake2b(np.ascontiguousarray(v).tobytes(), digest_size=16).hexdigest()
    return float(v).hex()


def main():
    out_file, with_oracle = sys.argv[1], sys.argv[2] == "1"
    import pllhip_ctypes as pc
    from test_gpu_parity import lnl_close, site_err, REL_CLV
    product = pc.PllLib(pc.PRODUCT_LIB)
    oracle = pc.PllLib(os.environ.get("PLLHIP_ORACLE_LIB") or os.path.join(ROOT, "oracle", "_build", "libpll_oracle.so")) \
        if with_oracle else None
    result = {}
    for case, (shape, ntips, nsites) in CASES.items():
        tree = make_tree(pc, shape, ntips)
        inst = pc.build_instance(product, states=20, rate_cats=4, ntips=ntips, nsites=nsites, coded=True, tree=tree)
        with inst:
            got, counters = observe(pc, inst, tree, shape, nsites)
        entry = {"counters": counters, "values": {name: digest(v) for name, v in got}}
        result[case] = entry
        if oracle is not None:
            ref_tree = make_tree(pc, shape, ntips)
            ref_inst = pc.build_instance(oracle, states=20, rate_cats=4, ntips=ntips, nsites=nsites, coded=True, tree=ref_tree)
            with ref_inst:
                ref, _ = observe(pc, ref_inst, ref_tree, shape, nsites)
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
            entry["oracle"] = True
    result["bench"] = bench_pattern(pc, product)
    with open(out_file, "w") as f:
        json.dump(result, f)


if __name__ == "__main__":
    main()
