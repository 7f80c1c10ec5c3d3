"""Sampled ancestral states on the device: pllhip_sample_ancestral_edges / _utree and pllhip_eval_sample_ancestral
(include/pllhip.h; contract: INTEGRATION.md, "Sampled ancestral states") against the numpy restatement of the contract
(tests/ancsample_reference.py) fed with what the engine itself holds -- byte for byte --, the storage forms the vectors
can have, the invariances the contract promises, the partition left alone, and the refusals.

The device driver is compared with the oracle's host path directly: both libraries load into one process (as in
tests/test_gpu_parity.py)."""
import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import pytest

import ancestral_reference as ar
import ancsample_reference as asr
import pllhip_ctypes as pc
import sitecat_reference as sr
from test_ancestral_exact import ambiguity_map

pytestmark = pytest.mark.gpu

TIPS, COMPONENT = pc.PLLHIP_ANCS_TIPS, pc.PLLHIP_ANCS_COMPONENT
CANARY = 0xA5


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
    "twentyfour_states": (24, 2, dict(ntips=6), {}),
    "protein_ladder": (20, 4, dict(ntips=12, ladder=True), {}),
    "protein_mixture": (20, 4, dict(ntips=9), dict(mixture=[0, 1, 2, 3], mixture_pinv=[0.1, 0.0, 0.3, 0.2])),
    "codon": (61, 4, dict(ntips=5), {}),
}


def constant_codes(ntips, nsites, states, seed=44):
    """random codes whose every seventh site holds one state at every tip, so that p-inv has sites to act on"""
    codes = pc.random_codes(ntips, nsites, states, seed)
    codes[:, ::7] = (np.arange(0, nsites, 7) % states)[None, :]
    return codes


def make(lib, name, nsites, tree=None, ambiguous=False, **more):
    """the instance of a shape after a full traversal towards its root edge"""
    S, R, tree_kw, kw = SHAPES[name]
    tree = tree or pc.Tree(seed_topology=61, seed_brlen=62, **tree_kw)
    inst = pc.build_instance(lib, S, R, tree.ntips, nsites, tree=tree, codes=constant_codes(tree.ntips, nsites, S),
                             **{**kw, **more})
    if ambiguous:
        cmap, (c1, c2) = ambiguity_map(S)
        rnd = pc.splitmix64(49, tree.ntips * nsites).reshape(tree.ntips, nsites)
        codes = constant_codes(tree.ntips, nsites, S)
        for t in range(tree.ntips):
            seq = (codes[t] + 48).astype(np.uint8)
            seq[rnd[t] % np.uint64(5) == 0] = ord("-")
            seq[rnd[t] % np.uint64(7) == 1] = ord(c1)
            seq[rnd[t] % np.uint64(11) == 2] = ord(c2)
            inst.set_tip_states(t, cmap, seq.tobytes())
        if inst.p.contents.invariant and not inst.L.pll_update_invariant_sites(inst.p):     # (they follow the tips)
            raise RuntimeError(lib.errmsg)
    pc.full_traversal(inst)
    return inst


def root_edge_of(inst):
    t = inst.tree
    sc = (lambda n: t.scaler_of(n)) if inst.nscalers else (lambda n: pc.PLL_SCALE_BUFFER_NONE)
    return t.root_a, sc(t.root_a), t.root_b, sc(t.root_b)


def edges_of(inst):
    return pc.tree_edges(inst.tree, inst.tree.root_a)


def run(inst, seed, replicates=1, edges=None, **kw):
    pa, ch, mi = edges_of(inst) if edges is None else edges
    return pc.sample_ancestral_edges(inst, root_edge_of(inst), pa, ch, mi, seed, replicates, **kw)


def reference(inst, seed, replicates, flags=0, first_replicate=0):
    x = asr.gather(inst, edges_of(inst), root_edge_of(inst), asr.device_table)
    return asr.sample(x, seed, replicates, first_replicate, tips=bool(flags & TIPS))


def check(inst, seed, replicates, flags):
    """one call against the reference; the call comes first, so that it meets the vectors as the traversal left them"""
    out, comp, dropped = run(inst, seed, replicates, flags=flags, component=np.full((replicates, inst.N), CANARY, np.uint8))
    want, wcomp, wdropped = reference(inst, seed, replicates, flags)
    assert out.shape == want.shape
    assert np.array_equal(out, want), np.argwhere(out != want)[:5]
    assert np.array_equal(comp, wcomp) if flags & COMPONENT else (comp == CANARY).all()
    assert dropped == wdropped
    return out, wcomp


# ---------------------------------------------------------------------------
# 1. bytes equal the reference
# ---------------------------------------------------------------------------
CASES = [("dna_g4_i", s) for s in (1, 31, 32, 33, 65, 257, 1027)] + \
        [("binary", 130), ("five_states", 257), ("twentyfour_states", 70), ("protein_ladder", 515), ("protein_mixture", 300),
         ("codon", 70)]


@pytest.mark.parametrize("flags", [0, TIPS | COMPONENT], ids=["inner", "tips-component"])
@pytest.mark.parametrize("name,sites", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_bytes_equal_the_reference(product, name, sites, flags):
    with make(product, name, sites) as inst:
        out, comp = check(inst, 7001, 3, flags)
        n = inst.tips
        assert (out[:, n:2 * n - 2] < inst.S).all() and (out[:, 2 * n - 2:] == 255).all()
        assert (out[:, :n] < inst.S).all() if flags & TIPS else (out[:, :n] == 255).all()
        if "pinv" in SHAPES[name][3] or "mixture_pinv" in SHAPES[name][3]:
            assert sites < 200 or (comp & 0x80).any()
        if flags & TIPS:            # plain codes: the tip rows are the alignment
            for t in range(n):
                assert (out[:, t] == np.argmax(ar.clv_of(inst, t)[:, 0, :], axis=1)[None, :]).all()


# ---------------------------------------------------------------------------
# 2. the forms a vector can have
# ---------------------------------------------------------------------------
OPTION_SHAPES = [("dna_g4_i", 1027), ("protein_ladder", 515)]
OPTION_IDS = [n for n, _ in OPTION_SHAPES]


@pytest.mark.parametrize("coded", [True, False], ids=["coded", "vectors"])
@pytest.mark.parametrize("name,sites", OPTION_SHAPES, ids=OPTION_IDS)
def test_ambiguous_tips(product, name, sites, coded):
    with make(product, name, sites, ambiguous=True, coded=coded) as inst:
        out, _ = check(inst, 7002, 2, TIPS | COMPONENT)
        ambiguous = 0
        for t in range(inst.tips):
            mask = ar.clv_of(inst, t)[:, 0, :] > 0
            assert mask[np.arange(sites)[None, :], out[:, t]].all()
            single = mask.sum(axis=1) == 1
            assert (out[:, t][:, single] == np.argmax(mask, axis=1)[single][None, :]).all()
            ambiguous += int((~single).sum())
        assert ambiguous > sites


@pytest.mark.parametrize("name,sites,ntips", [("dna_g4_i", 1027, 160), ("protein_ladder", 515, 90)], ids=OPTION_IDS)
def test_rate_scalers_on_a_deep_tree(product, name, sites, ntips):
    tree = pc.Tree(ntips, 61, 62, ladder=True)
    tree.brlens = tree.brlens * 8
    with make(product, name, sites, tree=tree, attributes=pc.PLL_ATTRIB_RATE_SCALERS, alpha=0.3) as inst:
        re_ = root_edge_of(inst)
        counts = sr.counts_of(inst, re_[1]) + sr.counts_of(inst, re_[3])
        assert (counts.min(axis=1) != counts.max(axis=1)).any()
        check(inst, 7003, 2, COMPONENT)


@pytest.mark.parametrize("name,sites", OPTION_SHAPES, ids=OPTION_IDS)
def test_site_repeats(product, name, sites):
    with make(product, name, sites, attributes=pc.PLL_ATTRIB_SITE_REPEATS) as inst:
        check(inst, 7004, 2, TIPS | COMPONENT)


@pytest.mark.parametrize("name,sites", OPTION_SHAPES, ids=OPTION_IDS)
def test_after_an_evaluate_only_traversal(product, name, sites):
    """the traversal left vectors out; the call stores them, as any reader does"""
    S, R, tree_kw, kw = SHAPES[name]
    tree = pc.Tree(seed_topology=61, seed_brlen=62, **tree_kw)
    with pc.build_instance(product, S, R, tree.ntips, sites, tree=tree, codes=constant_codes(tree.ntips, sites, S), **kw) as inst:
        assert inst.L.pllhip_set_transient(inst.p, 1)
        pc.full_traversal(inst)
        assert inst.L.pllhip_set_transient(inst.p, 0)
        check(inst, 7005, 2, COMPONENT)


def driver_case(lib, name, sites):
    S, R, tree_kw, kw = SHAPES[name]
    tree = pc.Tree(seed_topology=61, seed_brlen=62, **tree_kw)
    codes = constant_codes(tree.ntips, sites, S)
    ev = pc.Evaluation(lib, tree.newick(), nparts=1)
    placed = np.zeros_like(codes)
    for k in range(tree.ntips):
        placed[ev.tip_clv[k]] = codes[k]
    inst = pc.build_instance(lib, S, R, tree.ntips, sites, tree=tree, codes=placed, **kw)
    if not ev.L.pllhip_eval_set_partition(ev.ev, 0, inst.p, inst.params_p):
        raise RuntimeError(lib.errmsg)
    ev.parts.append(inst)
    return ev, inst


@pytest.mark.parametrize("name,sites", OPTION_SHAPES, ids=OPTION_IDS)
def test_driver_in_evaluate_only_mode(product, name, sites):
    ev, inst = driver_case(product, name, sites)
    with ev:
        ev.set_transient(1)
        ev.loglh()
        before = ev.loglh()
        root = ev.root_edge()
        got, = ev.sample_ancestral(7006, replicates=2, flags=TIPS)
        edges, root_edge = asr.driver_edges(ev)
        x = asr.gather(inst, edges, root_edge, asr.device_table)
        out, comp, dropped = asr.sample(x, 7006, 2, tips=True)
        assert np.array_equal(got.out, out) and np.array_equal(got.component, comp) and got.dropped == dropped
        assert ev.root_edge() == root and ev.loglh(incremental=True) == before and ev.loglh() == before


def test_device_driver_equals_the_host_path(product, oracle):
    """the same seed through both implementations: the HIP engine's kernel and the driver's plain C on the oracle.  (Their
    inputs agree to a rounding, not bit for bit; a draw would have to fall within that of a boundary to differ.)"""
    results = []
    for lib in (product, oracle):
        ev, inst = driver_case(lib, "protein_mixture", 300)
        with ev:
            ev.loglh()
            got, = ev.sample_ancestral(7007, replicates=3, flags=TIPS)
            results.append((got.out, got.component, got.dropped))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    assert results[0][2] == results[1][2] == 0


def test_utree_form(product):
    ev, inst = driver_case(product, "dna_g4_i", 257)
    with ev:
        ev.loglh()
        root = ev.L.pllhip_eval_root(ev.ev)
        if not root.contents.next:
            root = root.contents.back
        out, comp, dropped = pc.sample_ancestral_utree(inst, root, 7008, 2, flags=COMPONENT)
        got, = ev.sample_ancestral(7008, replicates=2)
        assert np.array_equal(out, got.out) and np.array_equal(comp, got.component) and dropped == got.dropped


# ---------------------------------------------------------------------------
# 3. invariances, bytewise
# ---------------------------------------------------------------------------
ALL = TIPS | COMPONENT


@pytest.fixture(scope="module", params=OPTION_SHAPES, ids=OPTION_IDS)
def base(request, product):
    """(instance, replicates [0, 11) with every row and the components) -- computed once, never changed"""
    name, sites = request.param
    inst = make(product, name, sites)
    out, comp, _ = run(inst, 99, 11, flags=ALL)
    out.setflags(write=False)
    comp.setflags(write=False)
    yield inst, out, comp
    inst.close()


def same(got, out, comp, reps=slice(None)):
    return np.array_equal(got[0], out[reps]) and np.array_equal(got[1], comp[reps])


def test_the_base_is_the_reference(base):
    inst, out, comp = base
    want, wcomp, _ = reference(inst, 99, 11, ALL)
    assert np.array_equal(out, want) and np.array_equal(comp, wcomp)


@pytest.mark.parametrize("blocks", [1, 2])
def test_block_cap(base, blocks):
    inst, out, comp = base
    with env(PLLHIP_ANCS_BLOCKS=blocks):
        assert same(run(inst, 99, 11, flags=ALL), out, comp)


def test_replicates_per_pass(base):
    inst, out, comp = base
    for cap in (1, 3):
        with env(PLLHIP_ANCS_REPLICATES=cap):
            assert same(run(inst, 99, 11, flags=ALL), out, comp)


def test_staging_chunks(base, product):
    inst, out, comp = base
    rows, sites = out.shape[1] + 1, out.shape[2]
    run(inst, 99, 11, flags=ALL)
    assert pc.ancsample_last_times(product)[3] == 1
    # room for two replicates per half: six chunks over replicates
    with env(PLLHIP_ANCS_STAGING_BYTES=4 * rows * ((sites + 3) // 4 * 4)):
        assert same(run(inst, 99, 11, flags=ALL), out, comp)
        assert pc.ancsample_last_times(product)[3] == 6
    # less than one replicate: site ranges of 256 columns
    with env(PLLHIP_ANCS_STAGING_BYTES=1):
        assert same(run(inst, 99, 11, flags=ALL), out, comp)
        assert pc.ancsample_last_times(product)[3] == 11 * ((sites + 255) // 256)


def test_replicate_range(base):
    inst, out, comp = base
    assert same(run(inst, 99, 3, first_replicate=2, flags=ALL), out, comp, slice(2, 5))
    assert same(run(inst, 99, 6, first_replicate=5, flags=ALL), out, comp, slice(5, 11))


def test_edge_order(base):
    inst, out, comp = base
    pa, ch, mi = edges_of(inst)
    perm = np.argsort(pc.splitmix64(5, len(pa)))
    assert not np.array_equal(perm, np.arange(len(pa)))
    assert same(run(inst, 99, 11, edges=(pa[perm], ch[perm], mi[perm]), flags=ALL), out, comp)
    rev = slice(None, None, -1)
    assert same(run(inst, 99, 11, edges=(pa[rev], ch[rev], mi[rev]), flags=ALL), out, comp)


def test_alphabet_and_unnamed_rows(base):
    inst, out, comp = base
    alphabet = "ACGT" if inst.S == 4 else "ARNDCQEGHILKMFPSTWYV"
    nodes = out.shape[1]
    got = run(inst, 99, 11, flags=ALL, alphabet=alphabet, node_count=nodes + 2)
    table = np.frombuffer(alphabet.encode(), dtype=np.uint8)
    want = np.where(out == 255, 255, table[np.minimum(out, inst.S - 1)])
    assert np.array_equal(got[0][:, :nodes], want) and np.array_equal(got[1], comp)
    assert (got[0][:, nodes:] == 255).all()


def test_the_partition_is_left_alone(base):
    inst, out, comp = base
    t = inst.tree
    re_ = root_edge_of(inst)
    nodes = range(2 * t.ntips - 2)
    before = ([inst.get_clv(n) for n in nodes], [inst.get_scaler(k) for k in range(inst.nscalers)],
              inst.edge_lnl(re_[0], re_[1], re_[2], re_[3], t.root_matrix))
    assert same(run(inst, 99, 11, flags=ALL), out, comp)
    after = ([inst.get_clv(n) for n in nodes], [inst.get_scaler(k) for k in range(inst.nscalers)],
             inst.edge_lnl(re_[0], re_[1], re_[2], re_[3], t.root_matrix))
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
    assert all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    assert before[2] == after[2]


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
        weights = np.ones(257, dtype=np.uint32)
        weights[np.flatnonzero(dead)[:2]] = 0
        inst.L.pll_set_pattern_weights(inst.p, weights.ctypes.data_as(pc.c_uint_p))
        out, comp = check(inst, 7009, 3, ALL)
        assert (out[:, :, dead] == 255).all() and (comp[:, dead] == 255).all() and (comp[:, ~dead] != 255).all()
        assert run(inst, 7009, 1)[2] == int(dead.sum()) - 2


# ---------------------------------------------------------------------------
# 4. refusals: the error is set and nothing is written
# ---------------------------------------------------------------------------
def test_refusals(base, product):
    inst, _, _ = base
    t = inst.tree
    pa, ch, mi = edges_of(inst)
    re_ = root_edge_of(inst)
    nodes = 2 * t.ntips - 2

    def refused(match, root_edge=re_, edges=(pa, ch, mi), **kw):
        out = np.full((kw.get("replicates", 1), kw.get("node_count", nodes), inst.N), CANARY, np.uint8)
        comp = np.full((kw.get("replicates", 1), inst.N), CANARY, np.uint8)
        product.errno = 0
        with pytest.raises(RuntimeError, match=match or None):
            pc.sample_ancestral_edges(inst, root_edge, edges[0], edges[1], edges[2], 1, out=out, component=comp,
                                      **{"replicates": 1, **kw})
        assert product.errno == pc.PLL_ERROR_PARAM_INVALID
        assert (out == CANARY).all() and (comp == CANARY).all()

    refused("replicates is 0", replicates=0)
    refused("2\\^32", replicates=2, first_replicate=2 ** 32 - 1)
    refused("unknown flags", flags=4)
    refused("alphabet", alphabet="AC")
    refused("out of range", freqs_indices=[0, 0, 9, 0])
    refused("out of range", root_edge=(nodes, re_[1], re_[2], re_[3]))
    refused("is a tip", root_edge=(0, pc.PLL_SCALE_BUFFER_NONE, re_[0], re_[1]))
    refused("out of range", node_count=nodes - 1)
    # lists simplan::build rejects
    refused("", edges=(np.append(pa, pa[-1]), np.append(ch, ch[-1]), np.append(mi, mi[-1])))        # a node reached twice
    refused("", edges=(pa[:-1], ch[:-1], mi[:-1]), flags=TIPS)                                     # a missing tip
    bad = mi.copy()
    bad[0] = 10 ** 6
    refused("", edges=(pa, ch, bad))                                                                # a matrix out of range
    # no edge, or more than one, from root_node to other_node
    refused("0 edges lead from root node", root_edge=(re_[0], re_[1], re_[0], re_[1]))
    keep = ~((pa == re_[0]) & (ch == re_[2]))
    refused("", edges=(pa[keep], ch[keep], mi[keep]))
    refused("scal", root_edge=(re_[0], 10 ** 6, re_[2], re_[3]))
    # invalid category weights
    w = inst.p.contents.rate_weights
    saved = w[1]
    w[1] = -0.5
    try:
        refused("weight 1")
    finally:
        w[1] = saved
    # NULLs
    prm = pc._ancs_params(1, 1, 0, 0, None)
    ubyte_p = C.POINTER(C.c_ubyte)
    out = np.full((1, nodes, inst.N), CANARY, np.uint8)
    args = [inst.p, C.byref(prm), re_[0], re_[1], re_[2], re_[3], len(pa), pa.ctypes.data_as(pc.c_uint_p),
            ch.ctypes.data_as(pc.c_uint_p), mi.ctypes.data_as(pc.c_uint_p), inst.params_p, nodes,
            out.ctypes.data_as(ubyte_p), None, None]
    for k in (0, 1, 7, 10, 12):
        a = list(args)
        a[k] = None
        product.errno = 0
        assert not inst.L.pllhip_sample_ancestral_edges(*a) and product.errno == pc.PLL_ERROR_PARAM_INVALID
    prm.flags = COMPONENT
    assert not inst.L.pllhip_sample_ancestral_edges(*args) and "component" in product.errmsg
    assert (out == CANARY).all()
    prm.flags = 0
    assert inst.L.pllhip_sample_ancestral_edges(*args) and not (out[:, t.ntips:] == CANARY).any()


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


def test_an_ascertainment_attribute_is_ignored(product):
    with make(product, "dna_g4_i", 130) as plain:
        want = run(plain, 7010, 2, flags=ALL)
    S, R, tree_kw, kw = SHAPES["dna_g4_i"]
    tree = pc.Tree(seed_topology=61, seed_brlen=62, **tree_kw)
    with pc.build_instance(product, S, R, tree.ntips, 130, tree=tree, codes=constant_codes(tree.ntips, 130, S),
                           attributes=pc.PLL_ATTRIB_AB_FLAG | pc.PLL_ATTRIB_AB_LEWIS, **kw) as inst:
        inst.set_asc(pc.PLL_ATTRIB_AB_LEWIS)
        pc.full_traversal(inst)
        got = run(inst, 7010, 2, flags=ALL)
        assert same(got, want[0], want[1]) and got[2] == 0
