"""Parsimony starting trees (pll_fastparsimony_init / _stepwise, pll_parsimony_destroy) and
pllhip_parsimony_tree_score against a numpy restatement of the contract in INTEGRATION.md ("Parsimony"):
Fitch state sets per tip and site, weighted count of empty intersections, the taxon order of pll_random,
insertion on the cheapest edge, ties to the smallest split key."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pllhip_ctypes as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLL_ERROR_STEPWISE_TIPS = 128
PLL_ERROR_NOT_IMPLEMENTED = 902
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------
# the numpy oracle: a tip is a uint64 state mask per site, a tree an adjacency dict
# ---------------------------------------------------------------------------
def fitch(a, b):
    inter = a & b
    empty = inter == 0
    return np.where(empty, a | b, inter), empty


class Rng:
    """pll_random_create / pll_random_getint (csrc/host/pll_random.c)"""

    def __init__(self, seed):
        self.s = (0x9E3779B97F4A7C15 * (seed + 1)) & M64

    def getint(self, maxval):
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        return z % maxval if maxval > 0 else 0


def taxon_order(tips, seed):
    order, r = list(range(tips)), Rng(seed)
    for i in range(tips - 1, 0, -1):
        j = r.getint(i + 1)
        order[i], order[j] = order[j], order[i]
    return order


def down_sets(adj, masks, w):
    """memoised Fitch set of the side of u seen from `frm`, plus its cost"""
    memo = {}

    def D(u, frm):
        key = (u, frm)
        if key not in memo:
            if len(adj[u]) == 1:
                memo[key] = (masks[u], 0)
            else:
                a, b = [v for v in adj[u] if v != frm]
                (da, ca), (db, cb) = D(a, u), D(b, u)
                f, empty = fitch(da, db)
                memo[key] = (f, ca + cb + int(w[empty].sum()))
        return memo[key]
    return D


def tree_cost(adj, masks, w, edge=None):
    """Fitch cost of the tree, evaluated at `edge` (any edge gives the same value)"""
    D = down_sets(adj, masks, w)
    u, v = edge if edge else next((u, vs[0]) for u, vs in adj.items())
    (du, cu), (dv, cv) = D(u, v), D(v, u)
    return cu + cv + int(w[fitch(du, dv)[1]].sum())


def edges_of(adj):
    return [(u, v) for u in adj for v in adj[u] if u < v]


def insertion_costs(adj, masks, w, taxon):
    D = down_sets(adj, masks, w)
    out = {}
    for u, v in edges_of(adj):
        f, _ = fitch(D(u, v)[0], D(v, u)[0])
        out[(u, v)] = int(w[(f & masks[taxon]) == 0].sum())
    return out


def side_tips(adj, u, frm, ntips):
    out, stack = [], [(u, frm)]
    while stack:
        x, p = stack.pop()
        if x < ntips:
            out.append(x)
        else:
            stack.extend((y, x) for y in adj[x] if y != p)
    return tuple(sorted(out))


def insert(adj, u, v, taxon, x):
    adj[u] = [x if y == v else y for y in adj[u]]
    adj[v] = [x if y == u else y for y in adj[v]]
    adj[x] = [u, v, taxon]
    adj[taxon] = [x]


def oracle_stepwise(masks_list, w_list, seed):
    """the tree (as a split set) and score of stepwise addition over several partitions"""
    ntips = len(masks_list[0])
    order = taxon_order(ntips, seed)
    x0 = ntips
    adj = {order[0]: [x0], order[1]: [x0], order[2]: [x0], x0: [order[0], order[1], order[2]]}
    nxt = ntips + 1
    for k in range(3, ntips):
        t = order[k]
        total = {}
        for masks, w in zip(masks_list, w_list):
            for e, c in insertion_costs(adj, masks, w, t).items():
                total[e] = total.get(e, 0) + c
        best = min(total.values())

        def key(e):
            u, v = e
            # the side of the edge without order[0]
            a = side_tips(adj, u, v, ntips)
            return a if order[0] not in a else side_tips(adj, v, u, ntips)
        u, v = min((e for e, c in total.items() if c == best), key=key)
        insert(adj, u, v, t, nxt)
        nxt += 1
    score = sum(tree_cost(adj, m, w) for m, w in zip(masks_list, w_list))
    return adj_splits(adj, ntips), score, adj


def adj_splits(adj, ntips):
    out = set()
    for u, v in edges_of(adj):
        s = frozenset(side_tips(adj, u, v, ntips))
        out.add(s if 0 not in s else frozenset(range(ntips)) - s)
    return out


def random_tree(ntips, seed):
    t = pc.Tree(ntips, seed_topology=seed)
    adj = {}
    for u, v in ([x if x < ntips else x + 1000 for x in e] for e in t.edges):   # (inner ids clear of tip ids)
        adj.setdefault(u, []).append(v)
        adj.setdefault(v, []).append(u)
    return t, adj


def random_masks(ntips, nsites, S, seed, ambiguous=0.1):
    """state index per tip and site, some sites of every tip an ambiguous set (one of 24 random sets, so that
    every alphabet stays within the 256 tip codes of PLL_ATTRIB_PATTERN_TIP)"""
    codes = pc.random_codes(ntips, nsites, S, seed=seed)
    masks = np.left_shift(np.uint64(1), codes.astype(np.uint64))
    amb = pc.uniform01(seed + 5, ntips * nsites).reshape(ntips, nsites) < ambiguous
    pool = pc.splitmix64(seed + 6, 24)
    if S < 64:
        pool &= np.uint64((1 << S) - 1)
    extra = pool[(pc.splitmix64(seed + 7, ntips * nsites) % np.uint64(24)).astype(np.int64)].reshape(ntips, nsites)
    return np.where(amb & (extra != 0), extra, masks)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 4, 20, 61])
def test_oracle_insertion_cost_is_full_rescoring(S):
    """the insertion-cost formula equals rescoring the tree with the taxon inserted, at every edge,
    and the Fitch cost is the same at every edge it is evaluated at"""
    ntips, nsites = 12, 300
    masks = random_masks(ntips, nsites, S, seed=S)
    w = (pc.splitmix64(S + 9, nsites) % np.uint64(5)).astype(np.int64)
    _, adj = random_tree(ntips - 1, seed=S + 1)
    base = tree_cost(adj, masks, w)
    for e in edges_of(adj):
        assert tree_cost(adj, masks, w, e) == base
    taxon = ntips - 1
    for (u, v), c in insertion_costs(adj, masks, w, taxon).items():
        new = {k: list(vs) for k, vs in adj.items()}
        insert(new, u, v, taxon, 10 ** 6)
        assert tree_cost(new, masks, w) == base + c


def test_product_exports_tree_score_and_oracle_keeps_stub(product_nogpu, oracle):
    assert hasattr(product_nogpu.lib, "pllhip_parsimony_tree_score")
    assert not hasattr(oracle.lib, "pllhip_parsimony_tree_score")
    inst = pc.Instance(oracle, 5, 4, 16, 1, clv_buffers=0, prob_matrices=1, scalers=False)
    with inst:
        assert not oracle.lib.pll_fastparsimony_init(inst.p)
        assert oracle.errno == PLL_ERROR_NOT_IMPLEMENTED


# ---------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------
def make_partition(lib, masks, S, weights=None, how="states", attributes=0, rate_cats=1, clv_buffers=0):
    """a partition of the pllmod_utree_create_parsimony shape (0 CLV buffers, 1 P-matrix, no scalers) whose tips
    hold `masks`: through pll_set_tip_states (a char per distinct mask) or pll_set_tip_clv"""
    ntips, nsites = masks.shape
    if how == "pattern":
        attributes |= pc.PLL_ATTRIB_PATTERN_TIP
    inst = pc.Instance(lib, ntips, S, nsites, rate_cats, attributes=attributes, clv_buffers=clv_buffers,
                       prob_matrices=1, scalers=False)
    if how in ("states", "pattern"):
        distinct = np.unique(masks)
        assert len(distinct) < 220
        charmap = np.zeros(256, dtype=np.uint64)
        chars = {}
        for i, m in enumerate(distinct):
            charmap[33 + i] = m
            chars[int(m)] = 33 + i
        lut = np.vectorize(lambda m: chars[int(m)], otypes=[np.uint8])
        for t in range(ntips):
            inst.set_tip_states(t, charmap, bytes(lut(masks[t])))
    else:
        bits = ((masks[..., None] >> np.arange(S, dtype=np.uint64)) & np.uint64(1)).astype(np.float64)
        for t in range(ntips):
            # any positive entry is "in the set"
            inst.set_tip_clv(t, bits[t] * (0.25 + pc.uniform01(t + 3, nsites * S).reshape(nsites, S)))
    if weights is not None:
        inst.set_pattern_weights(weights)
    return inst


def stepwise(lib, parts, seed, labels=None):
    L = lib.lib
    arr = (C.c_void_p * len(parts))(*parts)
    score = C.c_uint(0)
    lab = (C.c_char_p * len(labels))(*[s.encode() for s in labels]) if labels else None
    tree = L.pll_fastparsimony_stepwise(arr, lab, C.byref(score), len(parts), seed)
    return tree, score.value


def tree_score(lib, parts, tree):
    arr = (C.c_void_p * len(parts))(*parts)
    score = C.c_uint(0)
    assert lib.lib.pllhip_parsimony_tree_score(arr, len(parts), tree, C.byref(score)), lib.errmsg
    return score.value


def newick_of(lib, tree):
    ptr = lib.lib.pll_utree_export_newick(tree.contents.vroot, None)
    s = C.string_at(ptr).decode()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(ptr)
    return s


def check_stepwise(lib, insts, masks_list, w_list, seed):
    parts = [lib.lib.pll_fastparsimony_init(i.p) for i in insts]
    assert all(parts), lib.errmsg
    try:
        tree, score = stepwise(lib, parts, seed)
        assert tree, lib.errmsg
        try:
            assert lib.lib.pll_utree_check_integrity(tree)
            splits, want, _ = oracle_stepwise(masks_list, w_list, seed)
            assert pc.utree_splits(tree) == splits
            assert score == want
            assert tree_score(lib, parts, tree) == score
        finally:
            lib.lib.pll_utree_destroy(tree, None)
    finally:
        for p in parts:
            lib.lib.pll_parsimony_destroy(p)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
CASES = [  # (S, tips, sites, how, weighted, simulated)
    (2, 8, 700, "states", False, False),
    (2, 16, 1500, "clv", True, True),
    (4, 24, 3000, "pattern", True, True),
    (4, 13, 1000, "clv", False, False),
    (20, 40, 900, "states", True, True),
    (20, 11, 2000, "pattern", False, False),
    (61, 20, 400, "states", True, False),
    (61, 9, 300, "clv", False, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("S,tips,sites,how,weighted,simulated", CASES)
def test_stepwise_matches_oracle(product, S, tips, sites, how, weighted, simulated):
    if simulated:
        t = pc.Tree(tips, seed_topology=S + tips)
        codes = pc.simulated_codes(t, sites, S, seed=S + 3, scale=2.0)
        masks = np.left_shift(np.uint64(1), codes.astype(np.uint64))
        gap = pc.uniform01(S + 4, tips * sites).reshape(tips, sites) < 0.03
        masks = np.where(gap, np.uint64(M64 if S == 64 else (1 << S) - 1), masks)
    else:
        masks = random_masks(tips, sites, S, seed=S * 7 + tips)
    w = (pc.splitmix64(sites, sites) % np.uint64(7)).astype(np.uint32) + 1 if weighted else np.ones(sites, np.uint32)
    inst = make_partition(product, masks, S, weights=w if weighted else None, how=how)
    with inst:
        for seed in (1, 7, 12345):
            check_stepwise(product, [inst], [masks], [w.astype(np.int64)], seed)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 20])
def test_stepwise_ascertainment_partition(product, S):
    """the ascertainment-bias columns behind `sites` are no sites of the parsimony score"""
    tips, sites = 10, 500
    masks = random_masks(tips, sites, S, seed=31 + S, ambiguous=0.0)
    inst = make_partition(product, masks, S, attributes=pc.PLL_ATTRIB_AB_LEWIS, rate_cats=4)
    with inst:
        check_stepwise(product, [inst], [masks], [np.ones(sites, np.int64)], 3)


@pytest.mark.gpu
def test_stepwise_multipart(product):
    """two alphabets over the same taxa, two partitions on one device, a partition over two shards"""
    tips = 14
    m4, m20 = random_masks(tips, 800, 4, seed=1), random_masks(tips, 600, 20, seed=2)
    w4 = (pc.splitmix64(3, 800) % np.uint64(3)).astype(np.uint32) + 1
    a = make_partition(product, m4, 4, weights=w4, how="pattern")
    b = make_partition(product, m20, 20, how="states")
    L = product.lib
    assert L.pllhip_set_sharding(2, None)
    try:
        c = make_partition(product, m20, 20, how="states", rate_cats=4)
    finally:
        assert L.pllhip_set_sharding(0, None)
    with a, b, c:
        assert L.pllhip_shard_count(c.p) == 2
        check_stepwise(product, [a, b], [m4, m20], [w4.astype(np.int64), np.ones(600, np.int64)], 5)
        check_stepwise(product, [c], [m20], [np.ones(600, np.int64)], 5)
        check_stepwise(product, [a, c], [m4, m20], [w4.astype(np.int64), np.ones(600, np.int64)], 9)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [2, 4, 20, 61])
def test_tree_score_random_trees(product, S):
    tips, sites = 15, 700
    masks = random_masks(tips, sites, S, seed=50 + S)
    w = (pc.splitmix64(S, sites) % np.uint64(4)).astype(np.uint32)
    inst = make_partition(product, masks, S, weights=w, how="states")
    with inst:
        p = product.lib.pll_fastparsimony_init(inst.p)
        assert p, product.errmsg
        try:
            for k in range(20):
                t, adj = random_tree(tips, seed=1000 + k)
                nwk = t.newick(labels=[f"t{i}" for i in range(tips)])
                tree = product.lib.pll_utree_parse_newick_string(nwk.encode())
                assert tree
                for i in range(tree.contents.tip_count):
                    nd = tree.contents.nodes[i].contents
                    nd.clv_index = int(nd.label.decode()[1:])
                try:
                    assert tree_score(product, [p], tree) == tree_cost(adj, masks, w.astype(np.int64))
                finally:
                    product.lib.pll_utree_destroy(tree, None)
        finally:
            product.lib.pll_parsimony_destroy(p)


@pytest.mark.gpu
def test_lifecycle_and_errors(product):
    L = product.lib
    tips, sites = 12, 400
    masks = random_masks(tips, sites, 20, seed=77)
    inst = make_partition(product, masks, 20, how="states")
    p = L.pll_fastparsimony_init(inst.p)
    assert p, product.errmsg
    inst.close()                                 # the object outlives its partition
    labels = [f"taxon{i}" for i in range(tips)]
    t1, s1 = stepwise(product, [p], 42, labels)
    t2, s2 = stepwise(product, [p], 42, labels)
    assert t1 and t2 and s1 == s2
    assert newick_of(product, t1) == newick_of(product, t2)
    assert {t1.contents.nodes[i].contents.label.decode() for i in range(tips)} == set(labels)
    assert all(t1.contents.nodes[i].contents.clv_index == i for i in range(tips))
    assert sorted(t1.contents.nodes[i].contents.clv_index for i in range(tips, 2 * tips - 2)) == \
        list(range(tips, 2 * tips - 2))
    splits, want, _ = oracle_stepwise([masks], [np.ones(sites, np.int64)], 42)
    assert pc.utree_splits(t1) == splits and s1 == want
    L.pll_utree_destroy(t1, None)
    L.pll_utree_destroy(t2, None)
    # mismatched tip counts
    other = make_partition(product, random_masks(tips + 1, sites, 20, seed=78), 20)
    with other:
        q = L.pll_fastparsimony_init(other.p)
        assert q
        tree, _ = stepwise(product, [p, q], 1)
        assert not tree and product.errno == PLL_ERROR_STEPWISE_TIPS
        L.pll_parsimony_destroy(q)
    L.pll_parsimony_destroy(p)
    # fewer than 3 tips
    small = make_partition(product, random_masks(2, sites, 4, seed=79), 4)
    with small:
        q = L.pll_fastparsimony_init(small.p)
        assert q
        tree, _ = stepwise(product, [q], 1)
        assert not tree and product.errno == PLL_ERROR_STEPWISE_TIPS
        L.pll_parsimony_destroy(q)


@pytest.mark.gpu
def test_large_case_is_exact_and_deterministic(product):
    tips, sites, S = 200, 20000, 20
    t = pc.Tree(tips, seed_topology=5)
    codes = pc.simulated_codes(t, sites, S, seed=6)
    masks = np.left_shift(np.uint64(1), codes.astype(np.uint64))
    inst = make_partition(product, masks, S, how="pattern")
    with inst:
        p = product.lib.pll_fastparsimony_init(inst.p)
        assert p, product.errmsg
        try:
            t1, s1 = stepwise(product, [p], 11)
            t2, s2 = stepwise(product, [p], 11)
            assert t1 and t2 and s1 == s2
            assert newick_of(product, t1) == newick_of(product, t2)
            adj = {}
            for i in range(2 * tips - 2):
                nd = t1.contents.nodes[i]
                recs = [nd]
                while nd.contents.next and C.addressof(recs[-1].contents.next.contents) != C.addressof(nd.contents):
                    recs.append(recs[-1].contents.next)
                adj[nd.contents.clv_index] = [r.contents.back.contents.clv_index for r in recs]
            assert s1 == tree_cost(adj, masks, np.ones(sites, np.int64))
            product.lib.pll_utree_destroy(t1, None)
            product.lib.pll_utree_destroy(t2, None)
        finally:
            product.lib.pll_parsimony_destroy(p)


@pytest.mark.gpu
def test_c_client_follows_pll_modules(product, oracle, tmp_path):
    """tests/parsimony_client: pllmod_utree_create_parsimony's call sequence, then one likelihood traversal over
    the tree; lnL against the oracle on the same tree, score against numpy"""
    exe = tmp_path / "client"
    lib_dir = os.path.join(ROOT, "pll-modules_amd")
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "parsimony_client", "client.c"), "-o", str(exe),
                    "-L", lib_dir, "-lpll_hip", "-lm", f"-Wl,-rpath,{lib_dir}"], check=True)
    out = subprocess.run([str(exe), "24", "500", "9"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    fields = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    score, nwk, lnl = int(fields["score"]), fields["newick"], float(fields["lnl"])
    # the client's alignment: states (site * 7 + tip * 3 + site * tip) % 4 with every 11th entry a gap
    tips, sites = 24, 500
    codes = np.array([[(n * 7 + t * 3 + n * t) % 4 for n in range(sites)] for t in range(tips)], dtype=np.uint64)
    masks = np.left_shift(np.uint64(1), codes)
    gap = np.array([[(n + t) % 11 == 0 for n in range(sites)] for t in range(tips)])
    masks = np.where(gap, np.uint64(15), masks)
    splits, want, _ = oracle_stepwise([masks], [np.ones(sites, np.int64)], 9)
    assert score == want
    # lnL of the same tree through the oracle library
    L = oracle.lib
    tree = L.pll_utree_parse_newick_string(nwk.encode())
    assert tree
    try:
        for i in range(tips):
            nd = tree.contents.nodes[i].contents
            nd.clv_index = int(nd.label.decode()[1:])
        assert pc.utree_splits(tree) == splits
        ref = oracle_lnl(oracle, tree, masks)
    finally:
        L.pll_utree_destroy(tree, None)
    assert abs(lnl - ref) <= 1e-8 * abs(ref), (lnl, ref)


def oracle_lnl(lib, tree, masks):
    """JC, 1 rate category, every branch 0.1 (what the client does) on `tree` through `lib`"""
    L = lib.lib
    tips, sites = masks.shape
    inst = pc.Instance(lib, tips, 4, sites, 1, clv_buffers=tips - 2, prob_matrices=2 * tips - 3, scalers=True)
    with inst:
        inst.set_model(np.ones(6), np.full(4, 0.25), [1.0])
        bits = ((masks[..., None] >> np.arange(4, dtype=np.uint64)) & np.uint64(1)).astype(np.float64)
        for t in range(tips):
            inst.set_tip_clv(t, bits[t])
        t = tree.contents
        root = t.vroot if t.vroot.contents.next else t.vroot.contents.back
        L.pll_utree_reset_template_indices(root, tips)
        for i in range(tips):
            nd = t.nodes[i].contents
            nd.clv_index = int(nd.label.decode()[1:])
        ops = []

        def post(rec):
            if not rec.contents.next:
                return
            a, b = rec.contents.next.contents.back, rec.contents.next.contents.next.contents.back
            post(a)
            post(b)
            ops.append((rec.contents.clv_index, rec.contents.scaler_index, a.contents.clv_index,
                        a.contents.pmatrix_index, a.contents.scaler_index, b.contents.clv_index,
                        b.contents.pmatrix_index, b.contents.scaler_index))
        post(root)
        post(root.contents.back)
        mats = sorted({o[3] for o in ops} | {o[6] for o in ops} | {root.contents.pmatrix_index})
        inst.update_pmatrices(mats, [0.1] * len(mats))
        inst.update_partials(ops)
        bk = root.contents.back.contents
        return inst.edge_lnl(root.contents.clv_index, root.contents.scaler_index, bk.clv_index, bk.scaler_index,
                             root.contents.pmatrix_index)
