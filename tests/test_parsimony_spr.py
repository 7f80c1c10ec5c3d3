"""Parsimony SPR rounds (pll_fastparsimony_stepwise_spr_round) and taxon extension (pll_fastparsimony_stepwise_extend)
against a numpy restatement of the contract in INTEGRATION.md ("Parsimony"): node ids (tips their rows, inner nodes
N + rank of their clv index), the visit order of pll_random, the strict-improvement rule against the pruned subtree's
own edge, the allowed edges of a constrained round, ties to the smallest split key; extension as stepwise addition
from the given tree."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pllhip_ctypes as pc
from test_parsimony import (PLL_ERROR_NOT_IMPLEMENTED, PLL_ERROR_STEPWISE_TIPS, down_sets, fitch, insert,
                            insertion_costs, make_partition, newick_of, random_masks, side_tips, taxon_order,
                            tree_cost, tree_score)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLL_ERROR_PARAM_INVALID = 113


# ---------------------------------------------------------------------------
# the numpy oracle
# ---------------------------------------------------------------------------
def root_at(adj, r0):
    parent, stack = {r0: None}, [r0]
    while stack:
        u = stack.pop()
        for x in adj[u]:
            if x not in parent:
                parent[x] = u
                stack.append(x)
    return parent


def total_cost(adj, masks_list, w_list):
    return sum(tree_cost(adj, m, w) for m, w in zip(masks_list, w_list))


def oracle_round(adj, ntips, masks_list, w_list, seed, gid=None, check=False):
    """one round; returns (adjacency after it, cost, moves).  gid: constraint group per inner node id."""
    adj = {k: list(v) for k, v in adj.items()}
    moves = 0
    for v in taxon_order(2 * ntips - 2, seed):
        parent = root_at(adj, 0)
        c0 = adj[0][0]
        if v == 0 or v == c0:
            continue
        p = parent[v]
        pp = parent[p]
        s = next(x for x in adj[p] if x not in (v, pp))
        sub = set(side_tips_nodes(adj, v, p))
        tp = {k: list(vs) for k, vs in adj.items() if k != p and k not in sub}
        tp[s] = [pp if x == p else x for x in tp[s]]
        tp[pp] = [s if x == p else x for x in tp[pp]]
        par2 = root_at(tp, 0)
        dv = [down_sets(adj, m, w)(v, p)[0] for m, w in zip(masks_list, w_list)]
        Ds = [down_sets(tp, m, w) for m, w in zip(masks_list, w_list)]

        def ins(x):
            y = par2[x]
            return sum(int(w[(fitch(D(x, y)[0], D(y, x)[0])[0] & d) == 0].sum())
                       for D, d, w in zip(Ds, dv, w_list))
        g = gid[p] if gid is not None else None

        def allowed(x):
            if x == s:
                return False
            if gid is None:
                return True
            y = par2[x]
            return (x >= ntips and gid[x] == g) or (y >= ntips and gid[y] == g)
        cand = {x: ins(x) for x in tp if x != 0 and allowed(x)}
        if not cand:
            continue
        ref = ins(s)
        best = min(cand.values())
        if best >= ref:
            continue
        x = min((x for x, c in cand.items() if c == best), key=lambda x: side_tips(tp, x, par2[x], ntips))
        y = par2[x]
        before = total_cost(adj, masks_list, w_list) if check else None
        tp[x] = [p if z == y else z for z in tp[x]]
        tp[y] = [p if z == x else z for z in tp[y]]
        tp[p] = [x, y, v]
        for a in sub:
            tp[a] = list(adj[a])
        adj = tp
        moves += 1
        if check:
            assert total_cost(adj, masks_list, w_list) == before - ref + best
    return adj, total_cost(adj, masks_list, w_list), moves


def side_tips_nodes(adj, u, frm):
    out, stack = [], [(u, frm)]
    while stack:
        x, p = stack.pop()
        out.append(x)
        stack.extend((y, x) for y in adj[x] if y != p)
    return out


def oracle_extend(adj, ntips, tips_in, rowmap, masks_list, w_list, seed):
    """stepwise addition of the rows of clv indices tips_in .. ntips-1 to adj (nodes: tip rows, inner anything >=
    ntips); returns (adjacency, cost)"""
    adj = {k: list(v) for k, v in adj.items()}
    k = ntips - tips_in
    rows = [rowmap[tips_in + j] for j in taxon_order(k, seed)] if k else []
    r0 = min(x for x in adj if x < ntips)
    nxt = max(adj) + 1
    for t in rows:
        total = {}
        for masks, w in zip(masks_list, w_list):
            for e, c in insertion_costs(adj, masks, w, t).items():
                total[e] = total.get(e, 0) + c
        best = min(total.values())

        def key(e):
            u, v = e
            a = side_tips(adj, u, v, ntips)
            return a if r0 not in a else side_tips(adj, v, u, ntips)
        u, v = min((e for e, c in total.items() if c == best), key=key)
        insert(adj, u, v, t, nxt)
        nxt += 1
    return adj, total_cost(adj, masks_list, w_list)


def splits_of(adj, ntips):
    """splits as frozensets of tip ids, the side without tip 0"""
    out = set()
    for u in adj:
        for v in adj[u]:
            if u < v:
                s = frozenset(side_tips(adj, u, v, ntips))
                out.add(s if 0 not in s else frozenset(x for x in adj if x < ntips) - s)
    return out


def random_adj(ntips, seed):
    t = pc.Tree(ntips, seed_topology=seed)
    adj = {}
    for u, v in t.edges:
        adj.setdefault(u, []).append(v)
        adj.setdefault(v, []).append(u)
    return t, adj


# ---------------------------------------------------------------------------
# pll_utree_t helpers
# ---------------------------------------------------------------------------
def rings(tree):
    t = tree.contents
    out = []
    for i in range(t.tip_count + t.inner_count):
        nd = t.nodes[i]
        recs = [nd]
        r = nd.contents.next
        while r and C.addressof(r.contents) != C.addressof(nd.contents):
            recs.append(r)
            r = r.contents.next
        out.append(recs)
    return out


def tree_adj(tree, rowmap=None, base=None):
    """the round's node ids: tips their rows, inner nodes N (or base) + rank of their clv index"""
    rs = rings(tree)
    tips = [r[0].contents.clv_index for r in rs if len(r) == 1]
    inner = sorted(r[0].contents.clv_index for r in rs if len(r) > 1)
    idof = {c: (int(rowmap[c]) if rowmap is not None else c) for c in tips}
    idof.update({c: (base or len(tips)) + k for k, c in enumerate(inner)})
    return {idof[r[0].contents.clv_index]: [idof[x.contents.back.contents.clv_index] for x in r] for r in rs}


def records(tree):
    """(address, clv index) of every record"""
    return sorted((C.addressof(x.contents), x.contents.clv_index) for r in rings(tree) for x in r)


def pmatrix_indices(tree):
    seen, out = set(), []
    for r in rings(tree):
        for x in r:
            a, b = C.addressof(x.contents), C.addressof(x.contents.back.contents)
            if (b, a) not in seen:
                seen.add((a, b))
                out.append(x.contents.pmatrix_index)
    return sorted(out)


def parse_tree(lib, ntips, seed):
    """a random binary tree whose tip t has clv index t (inner nodes ntips .. in postorder)"""
    t = pc.Tree(ntips, seed_topology=seed)
    tree = lib.lib.pll_utree_parse_newick_string(t.newick(labels=[f"t{i}" for i in range(ntips)]).encode())
    assert tree
    for i in range(ntips):
        nd = tree.contents.nodes[i].contents
        nd.clv_index = int(nd.label.decode()[1:])
    return tree


def spr_round(lib, parts, tree, seed, rowmap=None, clv_valid=None):
    arr = (C.c_void_p * len(parts))(*parts)
    m = (C.c_uint * len(rowmap))(*[int(x) for x in rowmap]) if rowmap is not None else None
    cv = (C.c_int * len(clv_valid))(*clv_valid) if clv_valid is not None else None
    cost = C.c_uint(0)
    rc = lib.lib.pll_fastparsimony_stepwise_spr_round(tree, arr, len(parts), m, seed, cv, C.byref(cost))
    return rc, cost.value


def extend(lib, parts, tree, seed, labels=None, rowmap=None):
    arr = (C.c_void_p * len(parts))(*parts)
    m = (C.c_uint * len(rowmap))(*[int(x) for x in rowmap]) if rowmap is not None else None
    lab = (C.c_char_p * len(labels))(*[s.encode() for s in labels]) if labels else None
    score = C.c_uint(0)
    rc = lib.lib.pll_fastparsimony_stepwise_extend(tree, arr, len(parts), lab, m, seed, C.byref(score))
    return rc, score.value


def check_round(lib, parts, tree, masks_list, w_list, seed, rowmap=None, clv_valid=None, gid=None):
    """one round on the product and the oracle; in-place and integrity checks; returns (cost, moves)"""
    ntips = tree.contents.tip_count
    adj = tree_adj(tree, rowmap)
    before = records(tree)
    pm = pmatrix_indices(tree)
    nwk = newick_of(lib, tree)
    want_adj, want, moves = oracle_round(adj, ntips, masks_list, w_list, seed, gid)
    rc, cost = spr_round(lib, parts, tree, seed, rowmap, clv_valid)
    assert rc, lib.errmsg
    assert cost == want
    assert splits_of(tree_adj(tree, rowmap), ntips) == splits_of(want_adj, ntips)
    assert records(tree) == before
    assert lib.lib.pll_utree_check_integrity(tree)
    assert pmatrix_indices(tree) == pm
    if not moves:
        assert newick_of(lib, tree) == nwk
    return cost, moves


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_product_rejects_bad_arguments_without_device(product_nogpu):
    L = product_nogpu.lib
    cost = C.c_uint(0)
    assert not L.pll_fastparsimony_stepwise_spr_round(None, None, 1, None, 1, None, C.byref(cost))
    assert product_nogpu.errno == PLL_ERROR_PARAM_INVALID
    assert not L.pll_fastparsimony_stepwise_extend(None, None, 1, None, None, 1, C.byref(cost))
    assert product_nogpu.errno == PLL_ERROR_PARAM_INVALID
    tree = parse_tree(product_nogpu, 6, 3)
    try:
        nwk = newick_of(product_nogpu, tree)
        assert not L.pll_fastparsimony_stepwise_spr_round(tree, None, 1, None, 1, None, C.byref(cost))
        assert product_nogpu.errno == PLL_ERROR_PARAM_INVALID
        assert not L.pll_fastparsimony_stepwise_spr_round(tree, None, 1, None, 1, None, None)
        assert product_nogpu.errno == PLL_ERROR_PARAM_INVALID
        arr = (C.c_void_p * 1)(None)
        assert not L.pll_fastparsimony_stepwise_extend(tree, arr, 1, None, None, 1, C.byref(cost))
        assert product_nogpu.errno == PLL_ERROR_PARAM_INVALID
        assert not L.pll_fastparsimony_stepwise_extend(tree, arr, 0, None, None, 1, C.byref(cost))
        assert product_nogpu.errno == PLL_ERROR_PARAM_INVALID
        assert newick_of(product_nogpu, tree) == nwk
    finally:
        L.pll_utree_destroy(tree, None)


def test_oracle_keeps_stubs(oracle):
    L = oracle.lib
    cost = C.c_uint(0)
    assert not L.pll_fastparsimony_stepwise_spr_round(None, None, 1, None, 1, None, C.byref(cost))
    assert oracle.errno == PLL_ERROR_NOT_IMPLEMENTED
    assert not L.pll_fastparsimony_stepwise_extend(None, None, 1, None, None, 1, C.byref(cost))
    assert oracle.errno == PLL_ERROR_NOT_IMPLEMENTED


@pytest.mark.parametrize("S", [2, 4, 20])
def test_oracle_round_checks_itself(S):
    """every oracle move lowers the cost by exactly ref - best (a full rescoring), rounds never raise the cost,
    and a constrained round keeps every split of the constraint"""
    ntips, nsites = 14, 200
    masks = random_masks(ntips, nsites, S, seed=S + 40)
    w = (pc.splitmix64(S, nsites) % np.uint64(4)).astype(np.int64)
    _, adj = random_adj(ntips, seed=S)
    cost = total_cost(adj, [masks], [w])
    for seed in (1, 2):
        adj, c, _ = oracle_round(adj, ntips, [masks], [w], seed, check=True)
        assert c <= cost
        cost = c
    # constraint: contract every inner edge whose lower node id is even; groups are the components
    _, adj = random_adj(ntips, seed=S + 1)
    gid = constraint_groups(adj, ntips, lambda u, v: (u + v) % 3 == 0)
    keep = constraint_splits(adj, ntips, gid)
    for seed in (3, 4, 5):
        adj, _, _ = oracle_round(adj, ntips, [masks], [w], seed, gid=gid, check=True)
        assert keep <= splits_of(adj, ntips)


def test_oracle_extend_checks_itself():
    ntips, tips_in, nsites, S = 12, 7, 300, 4
    masks = random_masks(ntips, nsites, S, seed=5)
    w = np.ones(nsites, np.int64)
    _, adj = random_adj(tips_in, seed=9)
    adj = {(k if k < tips_in else k + 100): [x if x < tips_in else x + 100 for x in v] for k, v in adj.items()}
    out, cost = oracle_extend(adj, ntips, tips_in, list(range(ntips)), [masks], [w], 3)
    assert sorted(x for x in out if x < ntips) == list(range(ntips))
    assert all(len(v) == 3 for k, v in out.items() if k >= ntips)
    assert splits_of(adj, ntips) <= {frozenset(s & set(range(tips_in))) for s in splits_of(out, ntips)} | \
        {frozenset(range(tips_in)) - frozenset(s) for s in splits_of(out, ntips)}
    assert cost == tree_cost(out, masks, w)


def constraint_groups(adj, ntips, contract):
    """group id per inner node: the components of the inner-inner edges `contract` accepts (a multifurcating
    constraint and this tree as one of its resolutions)"""
    gid = {u: u for u in adj if u >= ntips}

    def find(u):
        while gid[u] != u:
            u = gid[u]
        return u
    for u in adj:
        for v in adj[u]:
            if u < v and u >= ntips and v >= ntips and contract(u, v):
                a, b = find(u), find(v)
                gid[max(a, b)] = min(a, b)
    return {u: find(u) for u in gid}


def constraint_splits(adj, ntips, gid):
    out = set()
    for u in adj:
        for v in adj[u]:
            if u < v and not (u >= ntips and v >= ntips and gid[u] == gid[v]):
                s = frozenset(side_tips(adj, u, v, ntips))
                out.add(s if 0 not in s else frozenset(range(ntips)) - s)
    return out


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
CASES = [  # (S, tips, sites, how, weighted)
    (2, 12, 600, "states", False),
    (4, 16, 1500, "pattern", True),
    (4, 10, 800, "clv", False),
    (20, 14, 700, "states", True),
    (61, 9, 300, "clv", True),
]


def data(S, tips, sites, weighted, seed):
    masks = random_masks(tips, sites, S, seed=seed)
    w = (pc.splitmix64(sites + seed, sites) % np.uint64(5)).astype(np.uint32) + 1 if weighted else \
        np.ones(sites, np.uint32)
    return masks, w


@pytest.mark.gpu
@pytest.mark.parametrize("S,tips,sites,how,weighted", CASES)
def test_unconstrained_rounds(product, S, tips, sites, how, weighted):
    masks, w = data(S, tips, sites, weighted, S * 3 + tips)
    inst = make_partition(product, masks, S, weights=w if weighted else None, how=how)
    L = product.lib
    with inst:
        p = L.pll_fastparsimony_init(inst.p)
        assert p, product.errmsg
        try:
            for seed in (1, 29):
                tree = parse_tree(product, tips, seed + S)
                try:
                    last = tree_cost(tree_adj(tree), masks, w.astype(np.int64))
                    for r in range(8):
                        cost, moves = check_round(product, [p], tree, [masks], [w.astype(np.int64)], seed + r)
                        assert cost <= last
                        assert cost == tree_score(product, [p], tree)
                        last = cost
                        if not moves:
                            break
                finally:
                    L.pll_utree_destroy(tree, None)
        finally:
            L.pll_parsimony_destroy(p)


@pytest.mark.gpu
@pytest.mark.parametrize("S,how", [(2, "states"), (4, "clv"), (20, "pattern"), (61, "states")])
def test_constrained_rounds_keep_the_constraint(product, S, how):
    """pllmod_utree_resolve_parsimony_multipart: a random binary resolution of a multifurcating tree, the map of
    every inner clv index to the node it resolves (tips to themselves), rounds until no gain"""
    tips, sites = 18, 500
    masks, w = data(S, tips, sites, True, S + 70)
    inst = make_partition(product, masks, S, weights=w, how=how)
    L = product.lib
    with inst:
        p = L.pll_fastparsimony_init(inst.p)
        assert p, product.errmsg
        try:
            for seed in (2, 5):
                tree = parse_tree(product, tips, seed * 11 + S)
                try:
                    adj = tree_adj(tree)
                    gid = constraint_groups(adj, tips, lambda u, v: (u * 7 + v + seed) % 3 != 0)
                    # the clv-index map: inner node id -> clv of its group's representative
                    inner = sorted(r[0].contents.clv_index for r in rings(tree) if len(r) > 1)
                    clv_of = {tips + k: c for k, c in enumerate(inner)}
                    cv = [0] * (max(inner) + 1)
                    for c in range(tips):
                        cv[c] = c
                    for u, g in gid.items():
                        cv[clv_of[u]] = clv_of[g]
                    keep = constraint_splits(adj, tips, gid)
                    best = 1 << 32
                    for r in range(10):
                        cost, _ = check_round(product, [p], tree, [masks], [w.astype(np.int64)], seed, None, cv, gid)
                        assert keep <= splits_of(tree_adj(tree), tips)
                        if cost >= best:
                            break
                        best = cost
                finally:
                    L.pll_utree_destroy(tree, None)
        finally:
            L.pll_parsimony_destroy(p)


@pytest.mark.gpu
def test_permuted_rows_and_batch_one(product):
    """tip_msa_idmap moves tip rows; PLLHIP_PARS_SPR_BATCH=1 gives the same trees and costs as the default batch"""
    tips, sites, S = 20, 900, 4
    masks, w = data(S, tips, sites, True, 91)
    rowmap = np.random.default_rng(4).permutation(tips)
    inst = make_partition(product, masks, S, weights=w, how="pattern")
    L = product.lib
    with inst:
        p = L.pll_fastparsimony_init(inst.p)
        assert p, product.errmsg
        try:
            out = []
            for batch in (None, "1"):
                if batch:
                    os.environ["PLLHIP_PARS_SPR_BATCH"] = batch
                try:
                    tree = parse_tree(product, tips, 8)
                    costs = [check_round(product, [p], tree, [masks], [w.astype(np.int64)], s, rowmap)[0]
                             for s in (3, 4)]
                    out.append((costs, newick_of(product, tree)))
                    L.pll_utree_destroy(tree, None)
                finally:
                    os.environ.pop("PLLHIP_PARS_SPR_BATCH", None)
            assert out[0] == out[1]
        finally:
            L.pll_parsimony_destroy(p)


@pytest.mark.gpu
@pytest.mark.parametrize("S,how,k", [(2, "states", 0), (4, "clv", 1), (20, "pattern", 6), (61, "states", 4)])
def test_extend(product, S, how, k):
    tips, sites = 14, 400
    T = tips - k
    masks, w = data(S, tips, sites, S != 2, S + k)
    inst = make_partition(product, masks, S, weights=w if S != 2 else None, how=how)
    L = product.lib
    labels = [f"new{j}" for j in range(k)]
    with inst:
        p = L.pll_fastparsimony_init(inst.p)
        assert p, product.errmsg
        try:
            for rowmap in (None, np.random.default_rng(S).permutation(tips)):
                rows = list(range(tips)) if rowmap is None else [int(x) for x in rowmap]
                tree = parse_tree(product, T, S + 3)
                try:
                    adj = tree_adj(tree, rows[:T], tips)
                    old = records(tree)
                    want_adj, want = oracle_extend(adj, tips, T, rows, [masks], [w.astype(np.int64)], 13)
                    rc, score = extend(product, [p], tree, 13, labels, rowmap)
                    assert rc, product.errmsg
                    assert score == want
                    t = tree.contents
                    assert (t.tip_count, t.inner_count, t.edge_count) == (tips, tips - 2, 2 * tips - 3)
                    assert L.pll_utree_check_integrity(tree)
                    assert splits_of(tree_adj(tree, rows), tips) == splits_of(want_adj, tips)
                    assert sorted(t.nodes[i].contents.clv_index for i in range(tips)) == list(range(tips))
                    assert sorted(t.nodes[i].contents.clv_index for i in range(tips, 2 * tips - 2)) == \
                        list(range(tips, 2 * tips - 2))
                    for i in range(2 * tips - 2 if k else 0):
                        assert t.nodes[i].contents.clv_index == i
                    for i in range(T, tips):
                        assert t.nodes[i].contents.label.decode() == labels[i - T]
                    new = {a for a, _ in records(tree)}
                    assert {a for a, _ in old} <= new
                    shift = {(a, c if c < T else c + k) for a, c in old}
                    assert shift <= set(records(tree))
                    assert pmatrix_indices(tree) == list(range(2 * tips - 3)) if k else True
                    assert tree_score(product, [p], tree) == score if rowmap is None else True
                finally:
                    L.pll_utree_destroy(tree, None)
        finally:
            L.pll_parsimony_destroy(p)


@pytest.mark.gpu
def test_extend_errors_leave_the_tree(product):
    L = product.lib
    tips, sites = 10, 300
    masks, _ = data(4, tips, sites, False, 3)
    inst = make_partition(product, masks, 4)
    with inst:
        p = L.pll_fastparsimony_init(inst.p)
        assert p, product.errmsg
        try:
            def attempt(tree, errno, **kw):
                nwk, recs = newick_of(product, tree), records(tree)
                rc, _ = extend(product, [p], tree, 1, **kw)
                assert not rc and product.errno == errno
                assert newick_of(product, tree) == nwk and records(tree) == recs
            big = parse_tree(product, tips + 1, 2)
            small = parse_tree(product, 2 + 1, 2)
            tree = parse_tree(product, 6, 2)
            try:
                attempt(big, PLL_ERROR_STEPWISE_TIPS)
                attempt(tree, PLL_ERROR_PARAM_INVALID, rowmap=[0] * tips)
                tree.contents.nodes[0].contents.clv_index = 7           # a tip outside 0 .. T-1
                attempt(tree, PLL_ERROR_PARAM_INVALID)
                tree.contents.nodes[0].contents.clv_index = int(tree.contents.nodes[0].contents.label.decode()[1:])
                rc, _ = extend(product, [p], small, 1)
                assert rc, product.errmsg
                rc, _ = spr_round(product, [p], tree, 1)
                assert not rc and product.errno == PLL_ERROR_STEPWISE_TIPS
            finally:
                for t in (big, small, tree):
                    L.pll_utree_destroy(t, None)
        finally:
            L.pll_parsimony_destroy(p)


@pytest.mark.gpu
def test_multipart_and_sharded(product):
    tips = 13
    m4, m20 = random_masks(tips, 700, 4, seed=11), random_masks(tips, 500, 20, seed=12)
    w4 = (pc.splitmix64(5, 700) % np.uint64(3)).astype(np.uint32) + 1
    a = make_partition(product, m4, 4, weights=w4, how="pattern")
    b = make_partition(product, m20, 20, how="states")
    L = product.lib
    assert L.pllhip_set_sharding(2, None)
    try:
        c = make_partition(product, m20, 20, how="states", rate_cats=4)
    finally:
        assert L.pllhip_set_sharding(0, None)
    ws = [w4.astype(np.int64), np.ones(500, np.int64)]
    with a, b, c:
        assert L.pllhip_shard_count(c.p) == 2
        pa, pb, pcs = (L.pll_fastparsimony_init(x.p) for x in (a, b, c))
        assert pa and pb and pcs, product.errmsg
        try:
            for parts, ml, wl in (([pa, pb], [m4, m20], ws), ([pcs], [m20], ws[1:]), ([pa, pcs], [m4, m20], ws)):
                tree = parse_tree(product, tips, 4)
                try:
                    check_round(product, parts, tree, ml, wl, 6)
                    check_round(product, parts, tree, ml, wl, 7)
                finally:
                    L.pll_utree_destroy(tree, None)
                tree = parse_tree(product, tips - 4, 5)
                try:
                    adj = tree_adj(tree, None, tips)
                    want_adj, want = oracle_extend(adj, tips, tips - 4, list(range(tips)), ml, wl, 2)
                    rc, score = extend(product, parts, tree, 2)
                    assert rc and score == want
                    assert splits_of(tree_adj(tree), tips) == splits_of(want_adj, tips)
                finally:
                    L.pll_utree_destroy(tree, None)
        finally:
            for x in (pa, pb, pcs):
                L.pll_parsimony_destroy(x)


@pytest.mark.gpu
def test_larger_round_is_deterministic(product):
    tips, sites, S = 100, 10000, 20
    t = pc.Tree(tips, seed_topology=21)
    codes = pc.simulated_codes(t, sites, S, seed=22)
    masks = np.left_shift(np.uint64(1), codes.astype(np.uint64))
    inst = make_partition(product, masks, S, how="pattern")
    L = product.lib
    with inst:
        p = L.pll_fastparsimony_init(inst.p)
        assert p, product.errmsg
        try:
            out = []
            for _ in range(2):
                tree = parse_tree(product, tips, 23)
                try:
                    rc, cost = spr_round(product, [p], tree, 5)
                    assert rc, product.errmsg
                    assert cost == tree_cost(tree_adj(tree), masks, np.ones(sites, np.int64))
                    out.append((cost, newick_of(product, tree)))
                finally:
                    L.pll_utree_destroy(tree, None)
            assert out[0] == out[1]
        finally:
            L.pll_parsimony_destroy(p)


@pytest.mark.gpu
def test_c_client_resolve_and_extend(product, tmp_path):
    """tests/parsimony_spr_client: a resolved multifurcating constraint through SPR rounds until no gain, and a
    tree extended by the taxa it lacks; scores against numpy, constraint splits kept"""
    exe = tmp_path / "client"
    lib_dir = os.path.join(ROOT, "pll-modules_amd")
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "parsimony_spr_client", "client.c"), "-o", str(exe),
                    "-L", lib_dir, "-lpll_hip", "-lm", f"-Wl,-rpath,{lib_dir}"], check=True)
    tips, sites = 24, 600
    out = subprocess.run([str(exe), str(tips), str(sites), "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    fields = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    codes = np.array([[(n * 5 + t * 3 + n * t) % 4 for n in range(sites)] for t in range(tips)], dtype=np.uint64)
    masks = np.left_shift(np.uint64(1), codes)
    gap = np.array([[(n + 2 * t) % 13 == 0 for n in range(sites)] for t in range(tips)])
    masks = np.where(gap, np.uint64(15), masks)
    w = np.ones(sites, np.int64)
    for name in ("resolve", "extend"):
        tree = product.lib.pll_utree_parse_newick_string(fields[name + "_newick"].encode())
        assert tree
        try:
            for i in range(tips):
                nd = tree.contents.nodes[i].contents
                nd.clv_index = int(nd.label.decode()[1:])
            adj = tree_adj(tree)
            assert int(fields[name + "_score"]) == tree_cost(adj, masks, w)
            if name == "resolve":
                assert int(fields["resolve_rounds"]) >= 1
                for blk in range(tips // 4):
                    split = frozenset(range(4 * blk, 4 * blk + 4))
                    assert (split if 0 not in split else frozenset(range(tips)) - split) in splits_of(adj, tips)
        finally:
            product.lib.pll_utree_destroy(tree, None)
