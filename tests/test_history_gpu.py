"""Sampled substitution histories on the device: pllhip_sample_histories_edges / _utree and
pllhip_eval_sample_histories (include/pllhip.h; contract: INTEGRATION.md, "Sampled substitution histories") against the
numpy restatement of the contract (tests/history_reference.py) fed with what the engine itself holds -- integer for
integer and byte for byte --, the storage forms the vectors can have, the invariances the contract promises, the
partition left alone, and the refusals.  Shapes and helpers are those of tests/test_ancsample_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import history_reference as hr
import pllhip_ctypes as pc
import sitecat_reference as sr
from test_ancsample_gpu import (CASES, OPTION_IDS, OPTION_SHAPES, SHAPES, constant_codes, driver_case, edges_of, env, make,
                                root_edge_of)
from test_history_cpu import branches_of

pytestmark = pytest.mark.gpu

TIPS, COMPONENT, SITES = pc.PLLHIP_ANCS_TIPS, pc.PLLHIP_ANCS_COMPONENT, pc.PLLHIP_HIST_SITES
ALL = TIPS | COMPONENT | SITES
CANARY = 0xA5
NAMES = ("out", "component", "counts", "units", "changes", "dropped_edges")


def lengths_of(inst, matrix):
    return np.asarray(inst.tree.brlens, dtype=np.float64)[np.asarray(matrix, dtype=np.int64)]


def run(inst, seed, replicates=1, edges=None, lengths=None, flags=ALL, **kw):
    pa, ch, mi = edges_of(inst) if edges is None else edges
    ln = lengths_of(inst, mi) if lengths is None else lengths
    return pc.sample_histories_edges(inst, root_edge_of(inst), pa, ch, mi, ln, seed, replicates, flags=flags, **kw)


def weights_of(inst):
    return np.array([inst.p.contents.pattern_weights[n] for n in range(inst.N)], dtype=np.int64)


def reference(lib, inst, seed, replicates, first_replicate=0, edges=None, root_edge=None, lengths=None):
    """(out with tip rows, component, dropped) of the engine's own ancestral draw, and the reference's histories from it"""
    pa, ch, mi = edges_of(inst) if edges is None else edges
    ln = lengths_of(inst, mi) if lengths is None else lengths
    out, comp, dropped = pc.sample_ancestral_edges(inst, root_edge or root_edge_of(inst), pa, ch, mi, seed, replicates,
                                                   first_replicate=first_replicate, flags=TIPS | COMPONENT)
    return (out, comp, dropped), hr.sample(hr.tables(lib, inst, ln), out, comp, (pa, ch, mi), weights_of(inst), seed,
                                           first_replicate)


def same(h, anc, ref):
    return (np.array_equal(h.out, anc[0]) and np.array_equal(h.component, anc[1]) and h.dropped == anc[2] and
            np.array_equal(h.counts, ref.counts) and np.array_equal(h.units, ref.units) and
            np.array_equal(h.changes, ref.changes) and np.array_equal(h.dropped_edges, ref.dropped_edges))


def check(lib, inst, seed, replicates):
    """one call against the reference; the call comes first, so that it meets the vectors as the traversal left them"""
    h = run(inst, seed, replicates)
    anc, ref = reference(lib, inst, seed, replicates)
    assert np.array_equal(h.counts, ref.counts), np.argwhere(h.counts != ref.counts)[:5]
    assert np.array_equal(h.units, ref.units), np.argwhere(h.units != ref.units)[:5]
    assert same(h, anc, ref)
    return h, ref


def equal(a, b, reps=slice(None), edges=slice(None)):
    return (np.array_equal(a.out, b.out[reps]) and np.array_equal(a.component, b.component[reps]) and
            all(np.array_equal(getattr(a, n), getattr(b, n)[reps][:, edges]) for n in NAMES[2:]))


# ---------------------------------------------------------------------------
# 1. the device equals the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,sites", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_integers_equal_the_reference(product, name, sites):
    with make(product, name, sites) as inst:
        h, ref = check(product, inst, 8001, 3)
        assert (ref.dropped_edges == 0).all() and (sites < 60 or h.counts.sum() > 0)
        assert (h.changes != 255).all() and (h.units.view(np.int64) >= 0).all()


# ---------------------------------------------------------------------------
# 2. the forms a vector can have
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("coded", [True, False], ids=["coded", "vectors"])
@pytest.mark.parametrize("name,sites", OPTION_SHAPES, ids=OPTION_IDS)
def test_ambiguous_tips(product, name, sites, coded):
    with make(product, name, sites, ambiguous=True, coded=coded) as inst:
        check(product, inst, 8002, 2)


@pytest.mark.parametrize("name,sites,ntips", [("dna_g4_i", 1027, 160), ("protein_ladder", 515, 90)], ids=OPTION_IDS)
def test_rate_scalers_on_a_deep_tree(product, name, sites, ntips):
    tree = pc.Tree(ntips, 61, 62, ladder=True)
    tree.brlens = tree.brlens * 8
    with make(product, name, sites, tree=tree, attributes=pc.PLL_ATTRIB_RATE_SCALERS, alpha=0.3) as inst:
        re_ = root_edge_of(inst)
        counts = sr.counts_of(inst, re_[1]) + sr.counts_of(inst, re_[3])
        assert (counts.min(axis=1) != counts.max(axis=1)).any()
        check(product, inst, 8003, 1)


@pytest.mark.parametrize("name,sites", OPTION_SHAPES, ids=OPTION_IDS)
def test_site_repeats(product, name, sites):
    with make(product, name, sites, attributes=pc.PLL_ATTRIB_SITE_REPEATS) as inst:
        check(product, inst, 8004, 2)


@pytest.mark.parametrize("name,sites", OPTION_SHAPES, ids=OPTION_IDS)
def test_after_an_evaluate_only_traversal(product, name, sites):
    S, R, tree_kw, kw = SHAPES[name]
    tree = pc.Tree(seed_topology=61, seed_brlen=62, **tree_kw)
    with pc.build_instance(product, S, R, tree.ntips, sites, tree=tree, codes=constant_codes(tree.ntips, sites, S), **kw) as inst:
        assert inst.L.pllhip_set_transient(inst.p, 1)
        pc.full_traversal(inst)
        assert inst.L.pllhip_set_transient(inst.p, 0)
        check(product, inst, 8005, 2)


def driver_reference(lib, ev, inst, seed, replicates):
    edges, lengths = branches_of(ev)
    anc, = ev.sample_ancestral(seed, replicates=replicates, flags=TIPS)
    t = hr.tables(lib, inst, lengths)
    return anc, hr.sample(t, anc.out, anc.component, edges, weights_of(inst), seed), t


@pytest.mark.parametrize("name,sites", OPTION_SHAPES, ids=OPTION_IDS)
def test_driver_in_evaluate_only_mode(product, name, sites):
    ev, inst = driver_case(product, name, sites)
    with ev:
        ev.set_transient(1)
        ev.loglh()
        before = ev.loglh()
        root = ev.root_edge()
        got, = ev.sample_histories(8006, replicates=2, flags=TIPS | SITES)
        anc, ref, t = driver_reference(product, ev, inst, 8006, 2)
        assert np.array_equal(got.out, anc.out) and np.array_equal(got.component, anc.component)
        assert all(np.array_equal(getattr(got, n), getattr(ref, n)) for n in NAMES[2:])
        c, d, total = hr.summary(t.tau[3], ref.counts[1, 3], ref.units[1, 3])
        assert np.array_equal(got.dwell[1, 3], d) and got.total[1, 3] == total
        assert ev.root_edge() == root and ev.loglh(incremental=True) == before and ev.loglh() == before


def test_device_driver_equals_the_host_path(product, oracle):
    """the same seed through both implementations: the HIP engine's kernels and the driver's plain C on the oracle.
    (Their matrices agree to a rounding, not bit for bit; a draw would have to fall within that of a boundary to
    differ.)"""
    results = []
    for lib in (product, oracle):
        ev, inst = driver_case(lib, "protein_mixture", 300)
        with ev:
            ev.loglh()
            got, = ev.sample_histories(8007, replicates=3, flags=TIPS | SITES)
            results.append(got)
    a, b = results
    assert all(np.array_equal(getattr(a, n), getattr(b, n)) for n in NAMES + ("dwell", "total"))
    assert a.dropped == b.dropped == 0


def test_utree_form(product):
    ev, inst = driver_case(product, "dna_g4_i", 257)
    with ev:
        ev.loglh()
        root = ev.L.pllhip_eval_root(ev.ev)
        if not root.contents.next:
            root = root.contents.back
        h = pc.sample_histories_utree(inst, root, 8008, 2, flags=COMPONENT | SITES)
        got, = ev.sample_histories(8008, replicates=2, flags=SITES)
        order = np.argsort(h.edge_matrix)
        assert np.array_equal(h.edge_matrix[order], np.arange(len(order)))
        assert np.array_equal(h.out, got.out) and np.array_equal(h.component, got.component) and h.dropped == got.dropped
        assert all(np.array_equal(getattr(h, n)[:, order], getattr(got, n)) for n in NAMES[2:])


# ---------------------------------------------------------------------------
# 3. no configuration shows in any output
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=OPTION_SHAPES, ids=OPTION_IDS)
def base(request, product):
    """(instance, replicates [0, 7) of everything) -- computed once, never changed"""
    name, sites = request.param
    inst = make(product, name, sites)
    h = run(inst, 199, 7)
    for n in NAMES:
        getattr(h, n).setflags(write=False)
    yield inst, h
    inst.close()


def test_the_base_is_the_reference(base, product):
    inst, h = base
    anc, ref = reference(product, inst, 199, 7)
    assert same(h, anc, ref)


def test_the_states_are_those_of_the_ancestral_draw(base):
    inst, h = base
    pa, ch, mi = edges_of(inst)
    alphabet = "ACGT" if inst.S == 4 else "ARNDCQEGHILKMFPSTWYV"
    for flags in (0, TIPS, COMPONENT, TIPS | COMPONENT):
        for abc in (None, alphabet):
            want = pc.sample_ancestral_edges(inst, root_edge_of(inst), pa, ch, mi, 199, 7, flags=flags, alphabet=abc,
                                             component=np.full((7, inst.N), CANARY, np.uint8))
            got = run(inst, 199, 7, flags=flags, alphabet=abc, fill=CANARY)
            assert np.array_equal(got.out, want[0]) and np.array_equal(got.component, want[1]) and got.dropped == want[2]
            assert np.array_equal(got.counts, h.counts) and np.array_equal(got.units, h.units) and got.changes is None
    # neither array is needed
    got = run(inst, 199, 7, flags=SITES, want_out=False, want_component=False)
    assert all(np.array_equal(getattr(got, n), getattr(h, n)) for n in NAMES[2:])


@pytest.mark.parametrize("blocks", [1, 2])
def test_block_cap(base, blocks):
    inst, h = base
    with env(PLLHIP_HIST_BLOCKS=blocks, PLLHIP_ANCS_BLOCKS=blocks):
        assert equal(run(inst, 199, 7), h)


def test_replicates_per_pass(base):
    inst, h = base
    for cap in (1, 3):
        with env(PLLHIP_ANCS_REPLICATES=cap):
            assert equal(run(inst, 199, 7), h)
        with env(PLLHIP_HIST_REPLICATES=cap):
            assert equal(run(inst, 199, 7), h)


def test_staging_chunks(base):
    inst, h = base
    rows, sites = h.out.shape[1] + 1 + h.counts.shape[1], h.out.shape[2]
    # room for two replicates per half: chunks over replicates
    with env(PLLHIP_ANCS_STAGING_BYTES=4 * rows * ((sites + 3) // 4 * 4)):
        assert equal(run(inst, 199, 7), h)
    # less than one replicate: site ranges of 256 columns
    with env(PLLHIP_ANCS_STAGING_BYTES=1):
        assert equal(run(inst, 199, 7), h)


def test_tables_in_memory(base):
    """the form partitions of more than 64 states would take: every lane adds to memory itself"""
    inst, h = base
    with env(PLLHIP_HIST_LDS_BYTES=1):
        assert equal(run(inst, 199, 7), h)


def test_replicate_range(base):
    inst, h = base
    assert equal(run(inst, 199, 3, first_replicate=2), h, slice(2, 5))
    assert equal(run(inst, 199, 2, first_replicate=5), h, slice(5, 7))


def test_edge_order(base):
    inst, h = base
    pa, ch, mi = edges_of(inst)
    perm = np.argsort(pc.splitmix64(5, len(pa)))
    assert not np.array_equal(perm, np.arange(len(pa)))
    assert equal(run(inst, 199, 7, edges=(pa[perm], ch[perm], mi[perm])), h, edges=perm)
    rev = np.arange(len(pa))[::-1]
    assert equal(run(inst, 199, 7, edges=(pa[rev], ch[rev], mi[rev])), h, edges=rev)


def test_the_partition_is_left_alone(base):
    inst, h = base
    t = inst.tree
    re_ = root_edge_of(inst)
    nodes = range(2 * t.ntips - 2)

    def state():
        return ([inst.get_clv(n) for n in nodes], [inst.get_scaler(k) for k in range(inst.nscalers)],
                [inst.get_pmatrix(m) for m in range(t.nedges)], inst.edge_lnl(re_[0], re_[1], re_[2], re_[3], t.root_matrix))

    before = state()
    assert equal(run(inst, 199, 7), h)
    after = state()
    for k in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(before[k], after[k]))
    assert before[3] == after[3]


# ---------------------------------------------------------------------------
# 4. more than 64 states, extreme lengths
# ---------------------------------------------------------------------------
def test_more_than_64_states(product):
    """A partition of 70 states is what this test is about; the engine makes none (pll_partition_create stops at 64),
    so the kernel form such a partition would run -- tables in memory, every lane adding itself -- is driven through
    its knob at the largest alphabet the engine has, 61 states, 5 tips, 70 sites, against the reference."""
    product.errno = 0
    assert not product.lib.pll_partition_create(5, 3, 70, 70, 1, 8, 2, 3, 0)
    with make(product, "codon", 70) as inst:
        with env(PLLHIP_HIST_LDS_BYTES=1):
            check(product, inst, 8009, 3)


def test_extreme_lengths(product):
    """one branch of length 0 (no jump anywhere) and one whose Poisson table has 1020 entries"""
    from test_history_cpu import near_cap_lambda
    import substmap_reference as smr
    tree = pc.Tree(seed_topology=61, seed_brlen=62, ntips=5)
    with pc.build_instance(product, 4, 1, 5, 19, tree=tree, codes=constant_codes(5, 19, 4)) as inst:
        pc.full_traversal(inst)
        mu, _ = pc.history_rate_table(product, *smr.eigen_of(inst, 0), 1, states=4)
        lam = near_cap_lambda(product, pc.PLLHIP_HIST_MAX_TABLE - 4)
        pa, ch, mi = edges_of(inst)
        zero = int(mi[np.flatnonzero(ch < 5)[0]])
        long_ = int(mi[np.flatnonzero(ch < 5)[1]])
        tree.brlens[zero], tree.brlens[long_] = 0.0, lam / mu
        pc.full_traversal(inst)
        h, ref = check(product, inst, 8010, 2)
        ez, el = int(np.flatnonzero(mi == zero)[0]), int(np.flatnonzero(mi == long_)[0])
        assert (h.changes[:, ez] == 0).all() and (h.counts[:, ez] == 0).all()
        assert ref.jumps[:, el].min() > 500 and (h.changes[:, el] == 254).all()
        # a little longer and the call is refused
        ln = lengths_of(inst, mi)
        ln[el] *= 1.05
        with pytest.raises(RuntimeError, match=f"edge {el} .*more than 1024"):
            run(inst, 8010, 1, lengths=ln)


def test_dropped_sites(product):
    """both pendant edges of a cherry have length 0: the sites at which its tips disagree have likelihood 0"""
    S, R, tree_kw, kw = SHAPES["dna_g4_i"]
    tree = pc.Tree(seed_topology=61, seed_brlen=62, **tree_kw)
    ta, tb, ma, mb = next((op[2], op[5], op[3], op[6]) for op in tree.ops if op[2] < tree.ntips and op[5] < tree.ntips)
    tree.brlens[ma] = tree.brlens[mb] = 0.0
    codes = pc.random_codes(tree.ntips, 257, S, 44)
    codes[tb, ::3] = codes[ta, ::3]
    with pc.build_instance(product, S, R, tree.ntips, 257, tree=tree, codes=codes, **kw) as inst:
        pc.full_traversal(inst)
        dead = codes[ta] != codes[tb]
        h, ref = check(product, inst, 8011, 3)
        assert (h.changes[:, :, dead] == 255).all() and (h.changes[:, :, ~dead] != 255).all()


# ---------------------------------------------------------------------------
# 5. refusals: the error is set and nothing is written
# ---------------------------------------------------------------------------
def test_refusals(base, product):
    inst, _ = base
    t = inst.tree
    pa, ch, mi = edges_of(inst)
    ln = lengths_of(inst, mi)
    re_ = root_edge_of(inst)
    nodes = 2 * t.ntips - 2

    def refused(match, root_edge=re_, edges=(pa, ch, mi), lengths=ln, **kw):
        product.errno = 0
        with pytest.raises(RuntimeError, match=match or None) as err:
            pc.sample_histories_edges(inst, root_edge, edges[0], edges[1], edges[2], lengths, 1,
                                      **{"replicates": 1, "flags": ALL, "fill": CANARY, **kw})
        assert product.errno == pc.PLL_ERROR_PARAM_INVALID
        left = err.value.partial
        assert all((getattr(left, n) == CANARY).all() for n in NAMES if getattr(left, n) is not None)

    # what the ancestral draw refuses
    refused("replicates is 0", replicates=0)
    refused("2\\^32", replicates=2, first_replicate=2 ** 32 - 1)
    refused("unknown flags", flags=4)
    refused("unknown flags", flags=1 << 9)
    refused("alphabet", alphabet="AC")
    refused("out of range", freqs_indices=[0, 0, 9, 0])
    refused("out of range", root_edge=(nodes, re_[1], re_[2], re_[3]))
    refused("is a tip", root_edge=(0, pc.PLL_SCALE_BUFFER_NONE, re_[0], re_[1]))
    refused("out of range", node_count=nodes - 1)
    refused("", edges=(np.append(pa, pa[-1]), np.append(ch, ch[-1]), np.append(mi, mi[-1])), lengths=np.append(ln, ln[-1]))
    refused("", edges=(pa[:-1], ch[:-1], mi[:-1]), lengths=ln[:-1])
    refused("0 edges lead from root node", root_edge=(re_[0], re_[1], re_[0], re_[1]))
    w = inst.p.contents.rate_weights
    saved = w[1]
    w[1] = -0.5
    try:
        refused("weight 1")
    finally:
        w[1] = saved
    # its own
    refused("branch lengths are NULL", lengths=None)
    for bad in (-1e-3, float("nan"), float("inf")):
        x = ln.copy()
        x[2] = bad
        refused("length of edge 2", lengths=x)
    x = ln.copy()
    x[1] = 1e4
    refused("edge 1 .*more than 1024", lengths=x)
    big = mi.copy()
    big[0] = 1 << 19
    refused("2\\^19", edges=(pa, ch, big))
    refused("out of range", params_indices=[0, 0, 9, 0])
    pw = inst.p.contents.pattern_weights
    saved = pw[0]
    pw[0] = 2 ** 31 - 8
    try:
        refused("2\\^31")
    finally:
        pw[0] = saved
    # NULLs
    prm = pc._ancs_params(1, 1, 0, 0, None)
    ull_p = C.POINTER(C.c_ulonglong)
    counts = np.zeros((1, len(pa), inst.S, inst.S), dtype=np.uint64)
    units = np.zeros((1, len(pa), inst.R, inst.S), dtype=np.uint64)
    de = np.zeros((1, len(pa)), dtype=np.uint64)
    args = [inst.p, C.byref(prm), re_[0], re_[1], re_[2], re_[3], len(pa), pa.ctypes.data_as(pc.c_uint_p),
            ch.ctypes.data_as(pc.c_uint_p), mi.ctypes.data_as(pc.c_uint_p), inst.params_p, nodes, inst.params_p,
            ln.ctypes.data_as(pc.c_double_p), None, None, None, counts.ctypes.data_as(ull_p), units.ctypes.data_as(ull_p),
            None, de.ctypes.data_as(ull_p)]
    for k in (0, 1, 7, 10, 12, 13, 17, 18, 20):
        a = list(args)
        a[k] = None
        product.errno = 0
        assert not inst.L.pllhip_sample_histories_edges(*a) and product.errno == pc.PLL_ERROR_PARAM_INVALID
    prm.flags = SITES
    assert not inst.L.pllhip_sample_histories_edges(*args) and "changes" in product.errmsg
    prm.flags = 0
    assert inst.L.pllhip_sample_histories_edges(*args) and counts.sum() > 0


def test_a_sharded_partition_is_refused(product):
    L = product.lib
    dev = (C.c_int * 2)(0, 0)
    assert L.pllhip_set_sharding(2, dev)
    try:
        inst = make(product, "dna_g4_i", 130)
    finally:
        assert L.pllhip_set_sharding(0, None)
    with inst:
        assert L.pllhip_shard_count(inst.p) == 2
        with pytest.raises(RuntimeError, match="sharded"):
            run(inst, 1)
