"""Simulated alignments on the device: pllhip_simulate_edges / pllhip_simulate_utree (include/pllhip.h; contract:
INTEGRATION.md, "Simulated alignments") against the numpy restatement of the contract (tests/simulate_reference.py)
fed with the device's own matrices -- byte for byte --, the invariances the contract promises, the sampler against the
engine's own per-site likelihoods, the partition left alone, and the errors."""
import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import pytest

import pllhip_ctypes as pc
import simulate_reference as sr

pytestmark = pytest.mark.gpu

INNER = pc.PLLHIP_SIM_INNER
PART_SITES = 8              # the partition's own alignment plays no part in a simulation


@contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# name: (states, rate categories, tree, build_instance keywords)
SHAPES = {
    "dna_g4_i": (4, 4, dict(ntips=7), dict(pinv=0.2)),
    "binary": (2, 1, dict(ntips=3), {}),
    "five_states": (5, 4, dict(ntips=12, balanced=True), {}),
    "protein_ladder": (20, 4, dict(ntips=12, ladder=True), {}),
    "protein_mixture": (20, 4, dict(ntips=9), dict(mixture=[0, 1, 2, 3], mixture_pinv=[0.1, 0.0, 0.3, 0.2])),
    "codon": (61, 4, dict(ntips=5), {}),
}


def make(lib, name, part_sites=PART_SITES):
    """the instance of a shape with its matrices requested (not necessarily launched yet)"""
    S, R, tree_kw, kw = SHAPES[name]
    tree = pc.Tree(seed_topology=61, seed_brlen=62, **tree_kw)
    inst = pc.build_instance(lib, S, R, tree.ntips, part_sites, tree=tree, **kw)
    inst.update_pmatrices(np.arange(tree.nedges), tree.brlens)
    return inst


def edges_of(inst):
    return pc.tree_edges(inst.tree)


def run(inst, seed, sites, replicates=1, edges=None, **kw):
    pa, ch, mi = edges_of(inst) if edges is None else edges
    return pc.simulate_edges(inst, inst.tree.ntips, pa, ch, mi, seed, sites, replicates, **kw)


def reference(inst, seed, sites, replicates, inner, **kw):
    t = inst.tree
    pmats = {m: inst.get_pmatrix(m) for m in range(t.nedges)}
    weights, pinv, freqs = sr.model_arrays(inst)
    edges = list(zip(*[a.tolist() for a in edges_of(inst)]))
    return sr.simulate(seed, sites, replicates, weights, pinv, freqs, pmats, t.ntips, edges, t.ntips, 2 * t.ntips - 2,
                       inner=inner, **kw)


# ---------------------------------------------------------------------------
# 1. bytes equal the reference
# ---------------------------------------------------------------------------
CASES = [("dna_g4_i", s) for s in (1, 63, 64, 65, 1027)] + [("binary", 130), ("five_states", 257),
                                                            ("protein_ladder", 515), ("protein_mixture", 300), ("codon", 70)]


@pytest.mark.parametrize("flags", [0, INNER], ids=["tips", "inner"])
@pytest.mark.parametrize("name,sites", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_bytes_equal_the_reference(product, name, sites, flags):
    with make(product, name) as inst:
        got = run(inst, 7001, sites, 3, flags=flags)
        want = reference(inst, 7001, sites, 3, bool(flags & INNER))
        assert got.shape == want.shape
        assert got.max() < inst.S
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]


# ---------------------------------------------------------------------------
# 2. invariances, bytewise
# ---------------------------------------------------------------------------
INVARIANT_SHAPES = [("dna_g4_i", 1027), ("protein_ladder", 515)]


@pytest.fixture(scope="module", params=INVARIANT_SHAPES, ids=[n for n, _ in INVARIANT_SHAPES])
def base(request, product):
    """(instance, sites, replicates [0, 5) of the full site range with inner rows) -- computed once, never changed"""
    name, sites = request.param
    inst = make(product, name)
    full = run(inst, 99, sites, 5, flags=INNER)
    full.setflags(write=False)
    yield inst, sites, full
    inst.close()


def test_replicate_range(base):
    inst, sites, full = base
    assert np.array_equal(run(inst, 99, sites, 3, first_replicate=2, flags=INNER), full[2:5])


def test_site_range(base):
    inst, sites, full = base
    assert np.array_equal(run(inst, 99, 100, 5, first_site=37, flags=INNER), full[:, :, 37:137])


@pytest.mark.parametrize("blocks", [1, 3])
def test_block_cap(base, blocks):
    inst, sites, full = base
    with env(PLLHIP_SIM_BLOCKS=blocks):
        assert np.array_equal(run(inst, 99, sites, 5, flags=INNER), full)


def test_staging_chunks(base, product):
    inst, sites, full = base
    rows = full.shape[1]
    assert pc.simulate_last_times(product)[3] >= 1
    run(inst, 99, sites, 5, flags=INNER)
    assert pc.simulate_last_times(product)[3] == 1
    # room for one replicate per half: five chunks over replicates
    with env(PLLHIP_SIM_STAGING_BYTES=2 * rows * ((sites + 3) // 4 * 4)):
        assert np.array_equal(run(inst, 99, sites, 5, flags=INNER), full)
        assert pc.simulate_last_times(product)[3] == 5
    # less than one replicate: site ranges of 1024 columns, two per replicate here
    with env(PLLHIP_SIM_STAGING_BYTES=1):
        assert np.array_equal(run(inst, 99, sites, 5, flags=INNER), full)
        assert pc.simulate_last_times(product)[3] == 5 * ((sites + 1023) // 1024)


def test_edge_order(base):
    inst, sites, full = base
    pa, ch, mi = edges_of(inst)
    perm = np.argsort(pc.splitmix64(5, len(pa)))
    assert not np.array_equal(perm, np.arange(len(pa)))
    assert np.array_equal(run(inst, 99, sites, 5, edges=(pa[perm], ch[perm], mi[perm]), flags=INNER), full)
    rev = slice(None, None, -1)
    assert np.array_equal(run(inst, 99, sites, 5, edges=(pa[rev], ch[rev], mi[rev]), flags=INNER), full)


def test_alphabet(base):
    inst, sites, full = base
    alphabet = "ACGT" if inst.S == 4 else "ARNDCQEGHILKMFPSTWYV"
    got = run(inst, 99, sites, 5, flags=INNER, alphabet=alphabet)
    table = np.frombuffer(alphabet.encode(), dtype=np.uint8)
    assert np.array_equal(got, table[full])


def test_tip_rows_without_inner(base):
    inst, sites, full = base
    got = run(inst, 99, sites, 5)
    assert got.shape[1] == inst.tips
    assert np.array_equal(got, full[:, :inst.tips])


def test_rows_of_unnamed_nodes(base):
    """node_count beyond the nodes the list names: their rows hold 0xFF, the others are unchanged"""
    inst, sites, full = base
    nodes = full.shape[1]
    got = run(inst, 99, sites, 5, flags=INNER, node_count=nodes + 2)
    assert got.shape[1] == nodes + 2
    assert np.array_equal(got[:, :nodes], full)
    assert (got[:, nodes:] == 0xFF).all()
    with env(PLLHIP_SIM_STAGING_BYTES=1):
        assert np.array_equal(run(inst, 99, sites, 5, flags=INNER, node_count=nodes + 2), got)


def test_two_runs(base):
    inst, sites, full = base
    assert np.array_equal(run(inst, 99, sites, 5, flags=INNER), full)
    assert not np.array_equal(run(inst, 100, sites, 5, flags=INNER), full)


@pytest.mark.parametrize("name,sites", INVARIANT_SHAPES, ids=[n for n, _ in INVARIANT_SHAPES])
def test_sharded_partition(product, name, sites):
    L = product.lib
    with make(product, name, part_sites=130) as plain:
        dev = (C.c_int * 2)(0, 0)
        assert L.pllhip_set_sharding(2, dev)
        try:
            shard = make(product, name, part_sites=130)
        finally:
            assert L.pllhip_set_sharding(0, None)
        with shard:
            assert L.pllhip_shard_count(shard.p) == 2 and L.pllhip_shard_count(plain.p) == 1
            assert np.array_equal(run(shard, 99, sites, 2, flags=INNER), run(plain, 99, sites, 2, flags=INNER))


def utree_edges(utree):
    """(root clv, parent, child, matrix, length) of a parsed tree walked from its vroot, written from the definition"""
    def addr(p):
        return C.addressof(p.contents)

    root = utree.contents.vroot
    pa, ch, mi, bl = [], [], [], []
    stack = [(root, True)]
    while stack:
        entry, is_root = stack.pop()
        if not entry.contents.next:
            continue
        n = entry if is_root else entry.contents.next
        while True:
            pa.append(n.contents.clv_index)
            ch.append(n.contents.back.contents.clv_index)
            mi.append(n.contents.pmatrix_index)
            bl.append(n.contents.length)
            stack.append((n.contents.back, False))
            n = n.contents.next
            if addr(n) == addr(entry):
                break
    return root, pa, ch, mi, bl


@pytest.mark.parametrize("name,sites", INVARIANT_SHAPES, ids=[n for n, _ in INVARIANT_SHAPES])
def test_utree_form(product, name, sites):
    L = product.lib
    with make(product, name) as a, make(product, name) as b:
        utree = L.pll_utree_parse_newick_string(a.tree.newick().encode())
        assert utree
        try:
            root, pa, ch, mi, bl = utree_edges(utree)
            assert len(pa) == a.tree.nedges and root.contents.clv_index >= a.tips
            # a: the library walks the tree and requests the matrices; b: the caller does both
            got = pc.simulate_utree(a, root, 99, sites, 2, flags=INNER, update_matrices=True)
            b.update_pmatrices(mi, bl)
            want = pc.simulate_edges(b, root.contents.clv_index, pa, ch, mi, 99, sites, 2, flags=INNER)
            assert np.array_equal(got, want)
            # ... and with the matrices as they stand now
            assert np.array_equal(pc.simulate_utree(a, root, 99, sites, 2, flags=INNER, update_matrices=False), want)
            # a tip as the root is refused
            tip = utree.contents.nodes[0]
            with pytest.raises(RuntimeError, match="inner node"):
                pc.simulate_utree(a, tip, 99, sites, 1)
            assert product.errno == pc.PLL_ERROR_PARAM_INVALID
        finally:
            L.pll_utree_destroy(utree, None)


# ---------------------------------------------------------------------------
# 3. the sampler draws what the likelihood evaluates
# ---------------------------------------------------------------------------
def test_pattern_counts_match_the_engines_site_likelihoods(product):
    """4 tips, DNA, GTR + G4 + I, 2^20 sites: the counts of the 256 column patterns against n exp(persite lnL) of a
    partition whose sites are the patterns; the condition and the seed of tests/test_simulate_reference.py"""
    with sr.pattern_instance(product, pc) as inst:
        t = inst.tree
        pc.full_traversal(inst)
        sa, sb = t.scaler_of(t.root_a), t.scaler_of(t.root_b)
        _, persite = inst.edge_lnl(t.root_a, sa, t.root_b, sb, t.root_matrix, persite=True)
        prob = np.exp(persite)
        assert abs(prob.sum() - 1.0) < 1e-9
        n = sr.STAT_SITES
        rows = run(inst, sr.STAT_SEED, n)[0]
        bad = sr.accept(sr.pattern_counts(rows), n * prob)
        assert bad == [], bad


# ---------------------------------------------------------------------------
# 4. the partition is left alone
# ---------------------------------------------------------------------------
def test_partition_is_left_alone(product):
    with make(product, "protein_ladder", part_sites=70) as inst:
        t = inst.tree
        lnl = pc.full_traversal(inst)
        sa, sb = t.scaler_of(t.root_a), t.scaler_of(t.root_b)
        clv = inst.get_clv(t.root_a).copy()
        scaler = inst.get_scaler(sa).copy()
        before = inst.counters()
        run(inst, 5, 515, 2, flags=INNER)
        after = inst.counters()
        assert after.partial_launches == before.partial_launches and after.partial_ops == before.partial_ops
        assert after.pmatrix_launches == before.pmatrix_launches and after.model_uploads == before.model_uploads
        assert np.array_equal(inst.get_clv(t.root_a), clv)
        assert np.array_equal(inst.get_scaler(sa), scaler)
        again = inst.edge_lnl(t.root_a, sa, t.root_b, sb, t.root_matrix)
        assert again == lnl
        assert inst.counters().partial_launches == before.partial_launches


def test_queued_matrices_are_flushed(product):
    """matrix requests still queued at the call are part of `the matrices as they stand`"""
    with make(product, "dna_g4_i") as inst:
        t = inst.tree
        first = run(inst, 3, 200)
        inst.update_pmatrices([2], [t.brlens[2] * 7.0])           # one request: it stays queued
        second = run(inst, 3, 200)
        assert not np.array_equal(first, second)
        assert np.array_equal(second, reference(inst, 3, 200, 1, False))


# ---------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------
def test_errors(product):
    with make(product, "dna_g4_i") as inst:
        tips, nodes = inst.tips, 2 * inst.tips - 2
        root = tips
        pa, ch, mi = edges_of(inst)
        good_list = (pa, ch, mi)
        canary = np.full((2, nodes, 50), 0xA5, dtype=np.uint8)

        def refused(match, root=root, pa=pa, ch=ch, mi=mi, sites=50, replicates=2, node_count=nodes, **kw):
            out = canary.copy()
            with pytest.raises(RuntimeError, match=match):
                pc.simulate_edges(inst, root, pa, ch, mi, 1, sites, replicates, node_count=node_count, out=out, **kw)
            assert product.errno == pc.PLL_ERROR_PARAM_INVALID
            assert np.array_equal(out, canary)
            # ... and a valid call goes through afterwards
            good = pc.simulate_edges(inst, tips, *good_list, 1, 50, 2, flags=INNER, out=canary.copy())
            assert good.max() < inst.S

        def with_edge(p, c, m):
            return dict(pa=np.append(pa, p), ch=np.append(ch, c), mi=np.append(mi, m))

        def without(k):
            return dict(pa=np.delete(pa, k), ch=np.delete(ch, k), mi=np.delete(mi, k))

        refused("sites is 0", sites=0)
        refused("replicates is 0", replicates=0)
        bad = mi.copy()
        bad[3] = inst.tree.nedges
        refused(r"edge 3: matrix index \d+ out of range", mi=bad)
        bad = ch.copy()
        bad[2] = nodes
        refused(rf"edge 2: node {nodes} out of range", ch=bad)
        refused(r"root node \d+ out of range", root=nodes + 4)
        refused(r"params index 1 of category 2 out of range", params_indices=[0, 0, 1, 0])
        refused(rf"node {int(ch[1])} is reached twice", **with_edge(root, ch[1], 0))
        refused(r"tip 1 used as a parent", node_count=nodes + 1, **with_edge(1, nodes, 0))
        refused(r"root node 0 is a tip", root=0)
        k = int(np.flatnonzero(ch >= tips)[0])                    # the edge into an inner node: its subtree floats
        refused(r"is never reached from root node", **without(k))
        k = int(np.flatnonzero(ch == 4)[0])
        refused(r"tip 4 is missing", **without(k))
        refused(r"tip 4 is missing", flags=INNER, **without(k))
        refused(r"alphabet has fewer than 4 characters", alphabet="ACG")
    # an ascertainment-bias attribute
    tree = pc.Tree(5, 61, 62)
    with pc.build_instance(product, 4, 4, 5, PART_SITES, tree=tree,
                           attributes=pc.PLL_ATTRIB_AB_FLAG | pc.PLL_ATTRIB_AB_LEWIS) as inst:
        inst.set_asc(pc.PLL_ATTRIB_AB_LEWIS)
        pa, ch, mi = pc.tree_edges(tree)
        out = np.full((1, 5, 20), 0xA5, dtype=np.uint8)
        with pytest.raises(RuntimeError, match="ascertainment"):
            pc.simulate_edges(inst, 5, pa, ch, mi, 1, 20, 1, out=out)
        assert product.errno == pc.PLL_ERROR_PARAM_INVALID
        assert (out == 0xA5).all()
