"""pllhip_distances_partition / pllhip_distances_msa / pllhip_distmat_* on the device (csrc/pll_distance_dev.hip)
against the numpy restatements of tests/distance_reference.py and tests/nj_reference.py.

Counts and compared sites: every integer equal.  p distances: bit-equal.  JC: within 4 * 2^-52 * |d| (one rounding
each for the quotient, the subtraction and the product, one ulp for each side's log).  ML: within 1e-8 d + 1e-10 of
the root the reference finds in long double.  Neighbour joining: the join list bit-equal to the restatement."""
import ctypes as C

import numpy as np
import pytest

import distance_reference as dr
import nj_reference as njr
import pllhip_ctypes as pc
import test_msa_stats_gpu as mg
import test_msa_stats_restatement as rs
from test_gpu_parity import lnl_close

pytestmark = pytest.mark.gpu

NAMES = {2: "bin", 4: "nt", 20: "aa", 61: "s61"}


def draw(product, S, T, L, seed):
    """(character map, rows [T][L], codes): the characters of tests/test_msa_stats_gpu.py -- gaps and ambiguities
    among them --, one all-gap taxon and two identical taxa where there is room"""
    _, cmap, chars = mg.alphabet(product, NAMES[S])
    rng = np.random.default_rng(seed)
    rows = mg.draw(rng, chars, T, L)
    if T >= 5:
        rows[2] = ord("-")
        rows[3] = rows[1]
    return cmap, rows, dr.codes_of_rows(rows, cmap, S)


def draw_weights(kind, L, seed):
    if kind == "ones":
        return None
    w = np.random.default_rng(seed).integers(1, 301, size=L).astype(np.uint32)
    w[L // 2] = 128
    w[0] = 70000
    return w


def matrices(product, form, rows, cmap, S, w, **kw):
    """a DistMat of `rows` through one of the three tip forms"""
    if form == "msa":
        return pc.distances_msa(product, rows, S, cmap, w, **kw)
    attrs = pc.PLL_ATTRIB_PATTERN_TIP if form == "coded" else 0
    vectors = rs._bits(rs.masks_of(rows, cmap), S).astype(np.float64) if form == "vectors" else None
    with mg.partition(product, rows, cmap, S, w, attributes=attrs, vectors=vectors) as inst:
        return pc.distances_partition(product, inst.p, **kw)


def check_counts(dm, N):
    T = N.shape[0]
    for i in range(T):
        for j in range(T):
            got = dm.counts(i, j)
            assert got is not None, (dm.lib.errno, dm.lib.errmsg)
            assert np.array_equal(got, N[i, j]), (i, j)


# ---------------------------------------------------------------------------------------------------------------------
# counts and the closed-form distances: states that make 16-row tiles straddle taxa, one and several tiles, one and
# several MFMA steps, weights above 127
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["ones", "random"])
@pytest.mark.parametrize("L", [1, 63, 65, 1531])
@pytest.mark.parametrize("T", [2, 5, 17, 33])
@pytest.mark.parametrize("S", [2, 4, 20, 61])
def test_counts_and_distances(product, S, T, L, weights):
    cmap, rows, codes = draw(product, S, T, L, 7 * S + 100 * T + L)
    w = draw_weights(weights, L, L + T)
    N = dr.counts(codes, w, S)
    assert N.max() < 2 ** 31
    n = dr.compared(codes, w)
    for form in ("msa", "coded", "vectors"):
        dm = matrices(product, form, rows, cmap, S, w, method=pc.DIST_P, flags=pc.DIST_KEEP_COUNTS)
        assert dm is not None, (form, product.errno, product.errmsg)
        with dm:
            assert dm.T == T
            check_counts(dm, N)
            assert np.array_equal(dm.compared(), n), form
            want = dr.p_matrix(N)
            assert dm.matrix().tobytes() == want.tobytes(), form
            assert dm.no_overlap == int((np.triu(n == 0, 1)).sum())
    dm = matrices(product, "msa", rows, cmap, S, w, method=pc.DIST_JC)
    assert dm is not None, (product.errno, product.errmsg)
    with dm:
        got, want = dm.matrix(), dr.jc_matrix(N, S)
        err = np.abs(got - want)
        print("largest JC error in units of 2^-52 |d|:", np.max(err / np.maximum(np.abs(want), 1e-300)) * 2.0 ** 52)
        assert np.all(err <= 4 * 2.0 ** -52 * np.abs(want))
        assert dm.counts(0, 1) is None and product.errno == pc.PLL_ERROR_PARAM_INVALID


def test_transposed_blocks_differ_and_are_right(product):
    """N_ij against N_ji on taxa that differ: a swap of the operands' row and column maps would pass a symmetric check"""
    S, T, L = 20, 5, 257
    cmap, rows, codes = draw(product, S, T, L, 3)
    N = dr.counts(codes, None, S)
    assert not np.array_equal(N[0, 1], N[0, 1].T) and not np.array_equal(N[0, 4], N[4, 0])
    with pc.distances_msa(product, rows, S, cmap, None, flags=pc.DIST_KEEP_COUNTS) as dm:
        for i, j in ((0, 1), (1, 0), (0, 4), (4, 0), (1, 4), (4, 1)):
            assert np.array_equal(dm.counts(i, j), N[i, j]), (i, j)
            assert np.array_equal(dm.counts(i, j), dm.counts(j, i).T)


def test_bands_chunks_and_repeats_give_the_same_bits(product):
    S, T, L = 20, 17, 1531
    cmap, rows, codes = draw(product, S, T, L, 11)
    w = draw_weights("random", L, 12)
    N = dr.counts(codes, w, S)
    with pc.distances_msa(product, rows, S, cmap, w, method=pc.DIST_JC, flags=pc.DIST_KEEP_COUNTS) as dm:
        first = (dm.matrix().tobytes(), dm.compared().tobytes())
        check_counts(dm, N)
    with pc.distances_msa(product, rows, S, cmap, w, method=pc.DIST_JC, flags=pc.DIST_KEEP_COUNTS) as dm:
        assert (dm.matrix().tobytes(), dm.compared().tobytes()) == first
    # one MFMA step per wave, whole table
    with pc.distances_msa(product, rows, S, cmap, w, method=pc.DIST_JC, flags=pc.DIST_KEEP_COUNTS, chunk_columns=64) as dm:
        assert (dm.matrix().tobytes(), dm.compared().tobytes()) == first
        check_counts(dm, N)
    # bands of three taxa (not a divisor of 17), and of one
    row_bytes = S * T * S * 4
    for band in (3, 1):
        with pc.distances_msa(product, rows, S, cmap, w, method=pc.DIST_JC, budget_bytes=band * row_bytes + 8,
                              chunk_columns=640) as dm:
            assert (dm.matrix().tobytes(), dm.compared().tobytes()) == first, band
    assert pc.distances_msa(product, rows, S, cmap, w, flags=pc.DIST_KEEP_COUNTS, budget_bytes=3 * row_bytes) is None
    assert product.errno == pc.PLL_ERROR_PARAM_INVALID


def test_errors(product):
    S, T, L = 4, 5, 65
    cmap, rows, codes = draw(product, S, T, L, 13)
    # a true probability-vector tip
    v = rs._bits(rs.masks_of(rows, cmap), S).astype(np.float64)
    v[1, 7] = [0.5, 0.25, 0.25, 0.0]
    with mg.partition(product, None, None, S, None, attributes=0, vectors=v) as inst:
        assert pc.distances_partition(product, inst.p) is None
        assert product.errno == pc.PLL_ERROR_PARAM_INVALID and "0 and 1" in product.errmsg
    # a sharded partition
    dev = (C.c_int * 2)(0, 0)
    assert product.lib.pllhip_set_sharding(2, dev)
    try:
        inst = mg.partition(product, draw(product, S, T, 257, 14)[1], cmap, S, None)     # (64 sites per shard at least)
    finally:
        product.lib.pllhip_set_sharding(0, None)
    with inst:
        assert product.lib.pllhip_shard_count(inst.p) == 2
        assert pc.distances_partition(product, inst.p) is None
        assert product.errno == pc.PLL_ERROR_PARAM_INVALID and "sharded" in product.errmsg
    # weights that add up to 2^31
    w = np.ones(L, dtype=np.uint32)
    w[[3, 40]] = 2 ** 30
    assert pc.distances_msa(product, rows, S, cmap, w) is None
    assert product.errno == pc.PLL_ERROR_PARAM_INVALID and "2^31" in product.errmsg
    with mg.partition(product, rows, cmap, S, w) as inst:
        assert pc.distances_partition(product, inst.p) is None
        assert product.errno == pc.PLL_ERROR_PARAM_INVALID
    # a character without a state
    bad = rows.copy()
    bad[3, 17] = ord("!")
    assert pc.distances_msa(product, bad, S, cmap, None) is None
    assert product.errno == rs.PLL_ERROR_MSA_MAP_INVALID
    assert "Unknown state ! at sequence 4 position 18" in product.errmsg, product.errmsg
    # the ML distance is for partitions; several rate matrices are not taken
    assert pc.distances_msa(product, rows, S, cmap, None, method=pc.DIST_ML) is None
    assert product.errno == pc.PLL_ERROR_PARAM_INVALID
    inst = pc.build_instance(product, states=4, rate_cats=4, ntips=6, nsites=64, mixture=[0, 1, 0, 1])
    with inst:
        assert pc.distances_partition(product, inst.p, method=pc.DIST_ML) is None
        assert product.errno == pc.PLL_ERROR_PARAM_INVALID and "rate matri" in product.errmsg


# ---------------------------------------------------------------------------------------------------------------------
# the ML distance
# ---------------------------------------------------------------------------------------------------------------------
def mutated_taxa(S, T, L, seed):
    """copies of one sequence, taxon t changed at a share of its sites between 0.02 and 0.5 (one taxon at 0.5: two
    such taxa are saturated under p-inv 0.2, and their maximum lies at max_dist)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, S, size=L)
    shares = [0.02, 0.04, 0.08, 0.12, 0.2, 0.5][:T]
    return np.stack([np.where(rng.uniform(size=L) < s, (base + rng.integers(1, S, size=L)) % S, base)
                     for s in shares]).astype(np.uint8)


def model_pair(product, oracle, S, T, L, subst, freqs, alpha, R, pinv, codes):
    """the same partition in the product and in the oracle"""
    out = []
    cmap = pc.state_charmap(S)
    for lib in (product, oracle):
        inst = pc.Instance(lib, T, S, L, R, attributes=pc.PLL_ATTRIB_PATTERN_TIP, scalers=False, prob_matrices=1,
                           clv_buffers=max(1, T - 2))
        inst.set_model(subst, freqs, lib.gamma_cats(alpha, R) if R > 1 else np.ones(1))
        for t in range(T):
            inst.set_tip_states(t, cmap, (codes[t] + 48).tobytes())
        if pinv > 0:
            inst.set_pinv(pinv)
        out.append(inst)
    return out


ML_MODELS = ["gtr_g4", "gtr_g4_pinv", "aa_g4"]


def ml_model(name):
    if name == "aa_g4":
        rng = np.random.default_rng(20)
        f = rng.uniform(0.5, 1.5, size=20)
        return 20, rng.uniform(0.2, 3.0, size=190), f / f.sum(), 0.8, 0.0
    return 4, pc.DNA_GTR_RATES, pc.DNA_FREQS, 2.0, (0.2 if name.endswith("pinv") else 0.0)


@pytest.mark.parametrize("name", ML_MODELS)
def test_ml_distances(product, oracle, name):
    S, subst, freqs, alpha, pinv = ml_model(name)
    T, L = 6, 400
    codes = mutated_taxa(S, T, L, 30 + S)
    a, b = model_pair(product, oracle, S, T, L, subst, freqs, alpha, 4, pinv, codes)
    with a, b:
        N = dr.counts(codes, None, S)
        want = dr.ml_matrix(dr.Model(b), N)
        off = want[np.triu_indices(T, 1)]
        assert np.all(off > 10 * 1e-6) and np.all(off < 10.0 / 2), off       # every pair is an interior maximum
        dm = pc.distances_partition(product, a.p, method=pc.DIST_ML)
        assert dm is not None, (product.errno, product.errmsg)
        with dm:
            got = dm.matrix()
            gap = np.abs(got - want)
            print("largest |d - d_ref| / d_ref:", np.max(gap[want > 0] / want[want > 0]))
            assert np.all(gap <= 1e-8 * want + 1e-10), (got, want)
            assert np.array_equal(got, got.T) and np.all(np.diag(got) == 0.0)
            assert np.array_equal(dm.compared(), dr.compared(codes, None))


def test_ml_bounds_and_no_overlap(product, oracle):
    """identical taxa: min_dist.  Taxa that differ everywhere under the JC model: max_dist.  No shared site: max_dist,
    and the pair is counted"""
    S, L = 4, 200
    rng = np.random.default_rng(40)
    base = rng.integers(0, S, size=L).astype(np.uint8)
    codes = np.stack([base, base, (base + 1 + rng.integers(0, 3, size=L)) % S, base, base]).astype(np.uint8)
    cmap, gap = pc.state_charmap(S), ord("-")
    rows = codes + 48
    rows[3, :L // 2] = gap
    rows[4, L // 2:] = gap
    for min_dist, max_dist in ((0.0, 0.0), (1e-4, 3.0)):
        lo, hi = (min_dist or 1e-6), (max_dist or 10.0)
        inst = pc.Instance(product, 5, S, L, 1, attributes=pc.PLL_ATTRIB_PATTERN_TIP, scalers=False, prob_matrices=1,
                           clv_buffers=3)
        with inst:
            inst.set_model(np.ones(6), np.full(4, 0.25), np.ones(1))
            for t in range(5):
                inst.set_tip_states(t, cmap, rows[t].tobytes())
            dm = pc.distances_partition(product, inst.p, method=pc.DIST_ML, min_dist=min_dist, max_dist=max_dist)
            assert dm is not None, (product.errno, product.errmsg)
            with dm:
                d = dm.matrix()
                assert d[0, 1] == lo and d[1, 0] == lo
                assert d[0, 2] == hi and d[1, 2] == hi
                assert d[3, 4] == hi and dm.no_overlap == 1 and dm.compared()[3, 4] == 0
                assert d[0, 3] == lo and d[0, 4] == lo


# ---------------------------------------------------------------------------------------------------------------------
# neighbour joining
# ---------------------------------------------------------------------------------------------------------------------
def check_nj(product, dist, splits=None):
    """join list bit-equal to the restatement; the tree's splits those of the joins (and `splits`)"""
    T = dist.shape[0]
    want_slots, want_lengths = njr.nj(dist)
    with pc.distmat_from_host(product, dist) as dm:
        got = dm.nj_joins()
        assert got is not None, (product.errno, product.errmsg)
        assert np.array_equal(got[0], want_slots)
        assert got[1].tobytes() == want_lengths.tobytes()
        labels = [f"taxon{t}" for t in range(T)]
        tree = dm.nj(labels)
        assert tree is not None, (product.errno, product.errmsg)
        try:
            assert product.lib.pll_utree_check_integrity(tree)
            t = tree.contents
            assert (t.tip_count, t.inner_count, t.edge_count) == (T, T - 2, 2 * T - 3)
            for i in range(T):
                nd = t.nodes[i].contents
                assert nd.clv_index == i and nd.label == labels[i].encode() and not nd.next
            got_splits = pc.utree_splits(tree)
            assert got_splits == njr.splits_of_joins(T, want_slots)
            if splits is not None:
                assert got_splits == splits
            # tip lengths: the join that takes the tip, negative ones clamped
            expect, is_tip = {}, [True] * T
            for q in range(T - 3):
                i, j = int(want_slots[2 * q]), int(want_slots[2 * q + 1])
                if is_tip[i]:
                    expect[i] = max(want_lengths[2 * q], 0.0)
                if is_tip[j]:
                    expect[j] = max(want_lengths[2 * q + 1], 0.0)
                is_tip[i] = False
            for s, l in zip(want_slots[2 * (T - 3):], want_lengths[2 * (T - 3):]):
                if is_tip[int(s)]:
                    expect[int(s)] = max(l, 0.0)
            assert all(t.nodes[i].contents.length == expect[i] for i in range(T))
        finally:
            product.lib.pll_utree_destroy(tree, None)
    return want_slots, want_lengths


@pytest.mark.parametrize("T", [4, 5, 7, 64, 65, 257])
def test_nj_additive(product, T):
    dist, splits = njr.random_tree(T, np.random.default_rng(400 + T))
    check_nj(product, dist, splits)


@pytest.mark.parametrize("seed", [1, 2])
def test_nj_noisy(product, seed):
    """noise below half the shortest branch: the topology still is the generating tree's"""
    T = 33
    rng = np.random.default_rng(seed)
    dist, splits = njr.random_tree(T, rng)
    noise = np.triu(rng.uniform(-0.01, 0.01, size=(T, T)), 1)
    check_nj(product, dist + noise + noise.T, splits)


def test_nj_all_equal(product):
    """every Q ties in every round: only the tie rule decides"""
    check_nj(product, np.ones((9, 9)) - np.eye(9))


@pytest.mark.parametrize("T", [3, 4])
def test_nj_smallest(product, T):
    rng = np.random.default_rng(T)
    dist, splits = njr.random_tree(T, rng)
    check_nj(product, dist, splits)


def test_nj_negative_lengths_are_clamped_in_the_tree_only(product):
    d = np.array([[0, 6, 5, 3, 3.0], [6, 0, 1, 2, 8], [5, 1, 0, 6, 9], [3, 2, 6, 0, 9], [3, 8, 9, 9, 0]])   # far from additive
    slots, lengths = njr.nj(d)
    assert lengths.min() < 0
    with pc.distmat_from_host(product, d) as dm:
        got = dm.nj_joins()
        assert np.array_equal(got[0], slots) and got[1].tobytes() == lengths.tobytes()
        tree = dm.nj()
        try:
            t = tree.contents
            assert [t.nodes[i].contents.length for i in range(5)] == [0.0, 0.0, 1.5, 1.5, 3.5]      # -0.5 twice
            assert product.lib.pll_utree_check_integrity(tree)
        finally:
            product.lib.pll_utree_destroy(tree, None)
    assert pc.distmat_from_host(product, np.full((4, 4), np.nan)) is None
    assert product.errno == pc.PLL_ERROR_PARAM_INVALID


# ---------------------------------------------------------------------------------------------------------------------
# end to end: alignment -> JC distances -> NJ tree -> likelihood
# ---------------------------------------------------------------------------------------------------------------------
def tree_of_utree(utree):
    """a pllhip_ctypes.Tree with the topology, lengths and indices of a pll_utree_t"""
    u = utree.contents
    T = u.tip_count
    tree = pc.Tree(T)
    edges, brlens = [None] * u.edge_count, np.zeros(u.edge_count)
    for i in range(u.tip_count + u.inner_count):
        rec = u.nodes[i]
        for _ in range(3 if rec.contents.next else 1):
            r = rec.contents
            edges[r.pmatrix_index] = sorted([r.clv_index, r.back.contents.clv_index])
            brlens[r.pmatrix_index] = r.length
            if r.next:
                rec = r.next
    tree.edges, tree.brlens, tree.nedges = edges, brlens, len(edges)
    tree.adj = {}
    for k, (a, b) in enumerate(edges):
        tree.adj.setdefault(a, []).append((b, k))
        tree.adj.setdefault(b, []).append((a, k))
    tree.set_root_edge(len(edges) - 1)
    return tree


def test_alignment_to_nj_tree_to_likelihood(product, oracle):
    T, L, S = 12, 300, 4
    codes = pc.simulated_codes(pc.Tree(T, 5, 6), L, S, seed=9)
    rows = codes + 48
    dm = pc.distances_msa(product, rows, S, pc.state_charmap(S), None, method=pc.DIST_JC)
    assert dm is not None, (product.errno, product.errmsg)
    with dm:
        utree = dm.nj([f"t{t}" for t in range(T)])
        assert utree is not None, (product.errno, product.errmsg)
        try:
            assert product.lib.pll_utree_check_integrity(utree)
            tree = tree_of_utree(utree)
        finally:
            product.lib.pll_utree_destroy(utree, None)
    a = pc.build_instance(product, states=S, rate_cats=4, ntips=T, nsites=L, codes=codes)
    b = pc.build_instance(oracle, states=S, rate_cats=4, ntips=T, nsites=L, codes=codes, tree=tree)
    with a, b:
        assert np.isfinite(pc.full_traversal(a))
        a.tree = tree                                  # the existing instance takes the neighbour-joining tree
        la, lb = pc.full_traversal(a), pc.full_traversal(b)
        assert np.isfinite(la) and lnl_close(la, lb, L, S), (la, lb)
