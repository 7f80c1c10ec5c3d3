"""pllhip_treeset_consensus on the device (csrc/pll_treeset_dev.hip, csrc/kernels_treeset.hpp: k_cs_*) against the
sequential definition restated in tests/test_consensus_restatement.py.

Every comparison is exact: the split words and their order, the trees per split, and supports bit-equal to the one
division c / B.

Shapes: T = 4 has one split or none; 33 two words and a one-bit tail, where the "union is every tip" test can go
wrong; 64 no tail; 68 has 65 splits per tree; 130 more than four words, so that a split takes eight lanes of a wave;
B = 70 puts more trees than a wave has lanes; B = 2 makes c = 1 exactly half."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pllhip_ctypes as pc
import test_consensus_restatement as cr
import test_tree_support_restatement as rs

pytestmark = pytest.mark.gpu

CUTS = [1.0, 0.75, 0.5, 0.3, 0.25, 0.0]


def make_trees(T, B, kind, seed=0):
    """near: copies of one tree, each with up to 2 + T / 4 leaves regrafted; random: drawn one by one; equal: B times
    one tree; two: one tree and a copy with two leaves regrafted"""
    rng = random.Random(7919 * T + 31 * B + seed)
    labels = rs.labels_for(T)
    base = rs.random_tree(labels, rng)
    if kind == "near":
        trees = [rs.moved(base, rng.randrange(3 + T // 4) if T > 4 else 0, rng) if T > 4 or b % 2 == 0
                 else rs.random_tree(labels, rng) for b in range(B)]
    elif kind == "random":
        trees = [rs.random_tree(labels, rng) for _ in range(B)]
    elif kind == "equal":
        trees = [rs.copy_tree(base) for _ in range(B)]
    else:
        ids = {l: i for i, l in enumerate(labels)}
        other = rs.moved(base, 2, rng)
        while set(rs.splits(other, ids)) == set(rs.splits(base, ids)):
            other = rs.moved(base, 2, rng)
        trees = [base, other]
    return labels, {l: i for i, l in enumerate(labels)}, trees


_expected = {}


def expected(T, B, kind, seed=0):
    """cut -> (words, trees per split, supports, candidates, distinct splits), computed once per case"""
    key = (T, B, kind, seed)
    if key not in _expected:
        labels, ids, trees = make_trees(T, B, kind, seed)
        out = {}
        for cut in CUTS:
            stats = {}
            held = cr.consensus(trees, ids, cut, stats)
            out[cut] = (cr.words_array(held, T), np.array([c for _, c in held], np.uint32),
                        np.array([c / B for _, c in held], np.float64), stats["candidates"], stats["distinct"])
        _expected[key] = out
    return _expected[key]


def device_results(lib, T, B, kind, seed=0, reverse=False, cuts=CUTS):
    """cut -> (words, trees, supports, (accepted tests, pair tests))"""
    labels, ids, trees = make_trees(T, B, kind, seed)
    out = {}
    with pc.TreeSet(lib, T, labels) as ts:
        assert ts.h, (lib.errno, lib.errmsg)
        for t in (reversed(trees) if reverse else trees):
            assert ts.add(rs.to_newick(t)), (lib.errno, lib.errmsg)
        for cut in cuts:
            got = ts.consensus(cut)
            assert got is not None, (cut, lib.errno, lib.errmsg)
            out[cut] = got + (ts.last_consensus_counts(),)
    return out


def assert_matches(got, want, T, B):
    for cut, (words, trees, support, counts) in got.items():
        w, t, s, ncand, distinct = want[cut]
        assert words.shape == w.shape and np.array_equal(words, w), (T, B, cut)
        assert np.array_equal(trees, t), (T, B, cut)
        assert support.tobytes() == s.tobytes(), (T, B, cut)
        if cut >= 0.5:
            assert counts == (0, 0), "a majority is taken as it stands"
        # never more than every candidate against every split a tree can hold
        assert counts[0] <= ncand * (T - 3) and counts[1] <= ncand * (ncand - 1) // 2


CASES = [(4, 1, "near"), (4, 3, "near"), (5, 3, "near"), (33, 5, "near"), (64, 5, "near"), (68, 70, "near"),
         (130, 3, "near"), (33, 1, "near"), (33, 2, "two"), (68, 4, "equal"), (33, 5, "random")]


@pytest.mark.parametrize("T,B,kind", CASES)
def test_against_the_restatement(product, T, B, kind):
    got, want = device_results(product, T, B, kind), expected(T, B, kind)
    assert_matches(got, want, T, B)
    labels, ids, trees = make_trees(T, B, kind)
    if B == 1 or kind == "equal":
        # every threshold returns the tree itself, ascending, with full support
        for cut in CUTS:
            assert np.array_equal(got[cut][0], rs.split_words(trees[0], ids)) and (got[cut][2] == 1.0).all()
        # T - 3 splits are held before the selection starts: no test at all, where D * (T - 3) were possible
        assert got[0.0][3] == (0, 0)
    if kind == "two":
        common = set(rs.splits(trees[0], ids)) & set(rs.splits(trees[1], ids))
        assert 0 < len(common) < T - 3
        for cut in (1.0, 0.75, 0.5):
            assert cr.from_words(got[cut][0]) == sorted(common, key=lambda s: rs.words_of(s, T)), "half is no majority"
        assert len(got[0.0][0]) == T - 3 and (got[0.0][1][:len(common)] == 2).all()
    if kind == "random":
        assert len(got[0.5][0]) == 0, "majority rule over random trees: the star"
        assert 0 < len(got[0.0][0]) < T - 3, "maximal, and yet not a binary tree"


def test_the_selection_stops_when_the_tree_is_resolved(product):
    """68 tips, 70 trees: the extended majority rule holds T - 3 splits long before the candidates run out"""
    T, B = 68, 70
    words, trees, support, counts = device_results(product, T, B, "near", cuts=[0.0])[0.0]
    _, _, _, ncand, distinct = expected(T, B, "near")[0.0]
    assert len(words) == T - 3 and ncand == distinct > 2 * (T - 3)
    assert 0 < counts[0] < distinct * (T - 3) and counts[1] > 0


CHILD = r"""
import json, sys
sys.path[:0] = [%r, %r]
import pllhip_ctypes as pc
import test_consensus_gpu as g
lib = pc.PllLib(pc.PRODUCT_LIB)
got = g.device_results(lib, %d, %d, %r)
print(json.dumps({str(cut): [w.tolist(), t.tolist(), s.tobytes().hex(), list(c)] for cut, (w, t, s, c) in got.items()}))
"""


def in_a_child(T, B, kind, **env):
    code = CHILD % (os.path.dirname(pc.__file__), os.path.dirname(os.path.abspath(__file__)), T, B, kind)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), check=True, capture_output=True,
                         text=True, timeout=300).stdout
    return json.loads(out.splitlines()[-1])


def assert_child_matches(child, want, T):
    for cut in CUTS:
        w, t, s, _, _ = want[cut]
        words, trees, support, counts = child[str(cut)]
        assert np.array_equal(np.array(words, np.uint32).reshape(len(words), (T + 31) // 32), w), cut
        assert trees == t.tolist() and support == s.tobytes().hex(), cut


@pytest.mark.parametrize("block", ["1", "2", "3", "64"])
def test_block_size_changes_nothing(product, block):
    """33 tips, 5 trees: more candidates than any of these blocks, so that rounds end inside runs of equal counts"""
    want = expected(33, 5, "near")
    assert want[0.0][3] > 64 and len(want[0.0][0]) > len(want[0.5][0])
    child = in_a_child(33, 5, "near", PLLHIP_CONSENSUS_BLOCK=block)
    assert_child_matches(child, want, 33)
    if block == "1":
        assert child["0.0"][3][1] == 0, "a round of one candidate has no pair"


def test_batch_size_changes_nothing(product):
    want = expected(68, 70, "near")
    assert_child_matches(in_a_child(68, 70, "near", PLLHIP_TREESET_BATCH="1"), want, 68)
    assert_matches(device_results(product, 68, 70, "near"), want, 68, 70)


def test_the_order_of_the_trees_changes_nothing(product):
    """the rank is by content: the ids of the split table, which follow the order of insertion, decide nothing"""
    for T, B in ((33, 5), (130, 3)):
        assert_matches(device_results(product, T, B, "near", reverse=True), expected(T, B, "near"), T, B)


def test_trees_added_after_a_consensus(product):
    labels, ids, trees = make_trees(33, 5, "near")
    with pc.TreeSet(product, 33, labels) as ts:
        for t in trees[:2]:
            assert ts.add(rs.to_newick(t))
        first = ts.consensus(0.0)
        assert cr.from_words(first[0]) == [s for s, _ in cr.consensus(trees[:2], ids, 0.0)]
        for t in trees[2:]:
            assert ts.add(rs.to_newick(t))
        for cut in (0.5, 0.0):
            assert np.array_equal(ts.consensus(cut)[0], expected(33, 5, "near")[cut][0])


def test_errors_leave_the_set_usable(product):
    lib = product
    labels, ids, trees = make_trees(33, 5, "near")
    want = expected(33, 5, "near")
    with pc.TreeSet(lib, 33, labels) as ts:
        lib.errno = 0
        assert ts.consensus(0.5) is None and lib.errno == pc.PLL_ERROR_PARAM_INVALID           # an empty set
        lib.errno = 0
        assert ts.consensus_newick(0.5) is None and lib.errno == pc.PLL_ERROR_PARAM_INVALID
        for t in trees:
            assert ts.add(rs.to_newick(t))
        for bad in (-0.01, 1.01, float("nan"), float("inf")):
            lib.errno = 0
            assert ts.consensus(bad) is None and lib.errno == pc.PLL_ERROR_PARAM_INVALID, bad
            lib.errno = 0
            assert ts.consensus_newick(bad) is None and lib.errno == pc.PLL_ERROR_PARAM_INVALID, bad
        assert lib.lib.pllhip_treeset_consensus(None, 0.5, None, None, None, None) == 0
        assert lib.errno == pc.PLL_ERROR_PARAM_INVALID
        assert ts.count == 5
        # only the count, no array
        import ctypes as C
        K = C.c_uint(77)
        assert lib.lib.pllhip_treeset_consensus(ts.h, 0.0, C.byref(K), None, None, None) == 1 and K.value == len(want[0.0][0])
        for cut in CUTS:
            words, counts, support = ts.consensus(cut)
            assert np.array_equal(words, want[cut][0]) and support.tobytes() == want[cut][2].tobytes()
        up, kernel, down = ts.last_times()
        assert up >= 0 and kernel > 0 and down > 0
        # the other queries go on as before
        assert np.array_equal(ts.splits(0), rs.split_words(trees[0], ids))


@pytest.mark.parametrize("T,B,kind", [(4, 3, "near"), (33, 5, "near"), (33, 5, "random"), (68, 4, "equal")])
def test_consensus_newick(product, T, B, kind):
    """the tree parses back and has the splits and supports that the split system has"""
    lib = product
    labels, ids, trees = make_trees(T, B, kind)
    with pc.TreeSet(lib, T, labels) as ts:
        for t in trees:
            assert ts.add(rs.to_newick(t))
        for cut in (1.0, 0.5, 0.0):
            words, counts, support = ts.consensus(cut)
            newick = ts.consensus_newick(cut)
            assert newick, (lib.errno, lib.errmsg)
            got, inner = cr.tree_splits(newick, ids)
            assert got == set(cr.from_words(words)), (T, cut)
            assert inner == sorted(support.tolist())
            t = lib.lib.pll_utree_parse_newick_string(newick.encode())
            assert t, lib.errmsg
            assert (t.contents.tip_count, t.contents.inner_count) == (T, len(words) + 1)
            lib.lib.pll_utree_destroy(t, None)
