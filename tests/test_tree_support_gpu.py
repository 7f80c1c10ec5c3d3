"""pllhip_treeset_* on the device (csrc/pll_treeset_dev.hip, csrc/kernels_treeset.hpp) against the brute-force
restatement of tests/test_tree_support_restatement.py.

Every comparison is exact: split words equal, RF distances equal, the integers behind the supports (trees per split,
sum of transfer distances) equal, supports bit-equal to the restatement's single division.

Shapes: T = 4 has one split; 33 two words and a one-bit tail; 64 no tail; 68 has 65 reference splits, so a second wave
with one live lane; 130 more than one group of 64 splits and more than four words; a 200-tip caterpillar and a 256-tip
balanced tree test the order of the transfer program; B = 70 puts more trees than a wave has lanes."""
import json
import random

import numpy as np
import pytest

import pllhip_ctypes as pc
import test_tree_support_restatement as rs

pytestmark = pytest.mark.gpu


def make_case(T, B, shape="random", seed=0):
    """(labels, ids, reference tree, B trees): the first tree equals the reference, the next few are one to three
    moves away from it, the last is drawn on its own"""
    rng = random.Random(1000 * T + B + seed)
    labels = rs.labels_for(T)
    order = labels[:]
    rng.shuffle(order)
    ref = {"random": rs.random_tree, "caterpillar": lambda l, r: rs.caterpillar(l),
           "balanced": lambda l, r: rs.balanced(l)}[shape](order, rng)
    trees = []
    for b in range(B):
        if b == B - 1 and B > 1:
            trees.append(rs.random_tree(labels, rng))
        else:
            trees.append(rs.moved(ref, b % 4, rng) if T > 4 or b == 0 else rs.random_tree(labels, rng))
    return labels, {l: i for i, l in enumerate(labels)}, ref, trees


_expected = {}


def expected(key, labels, ids, ref, trees):
    """the restatement's results, computed once per case"""
    if key not in _expected:
        B, R = len(trees), len(ids) - 3
        have, of_ref = [set(rs.splits(t, ids)) for t in trees], set(rs.splits(ref, ids))
        _expected[key] = dict(
            splits=[rs.split_words(t, ids) for t in trees],
            rf_matrix=np.array([[2 * (R - len(a & b)) for b in have] for a in have], dtype=np.uint32).reshape(B, B),
            rf_to=np.array([2 * (R - len(of_ref & h)) for h in have], dtype=np.uint32),
            fbp=rs.fbp_set(ref, trees, ids), tbe=rs.tbe_set(ref, trees, ids))
    return _expected[key]


def results(lib, labels, ref, trees, all_splits=True):
    """everything the tree set computes, in one dictionary of arrays"""
    with pc.TreeSet(lib, len(labels), labels) as ts:
        assert ts.h, (lib.errno, lib.errmsg)
        for t in trees:
            assert ts.add(rs.to_newick(t)), (lib.errno, lib.errmsg)
        assert ts.count == len(trees)
        out = {"splits": []}
        for b in range(len(trees) if all_splits else min(3, len(trees))):
            w = ts.splits(b)
            assert w is not None, (lib.errno, lib.errmsg)
            out["splits"].append(w)
        out["rf_matrix"] = ts.rf_matrix()
        out["rf_to"] = ts.rf_to(rs.to_newick(ref))
        out["fbp"] = ts.support(rs.to_newick(ref), pc.SUPPORT_FBP)
        out["tbe"] = ts.support(rs.to_newick(ref), pc.SUPPORT_TBE)
        out["counts"] = ts.last_counts()
        for key in ("rf_matrix", "rf_to", "fbp", "tbe"):
            assert out[key] is not None, (key, lib.errno, lib.errmsg)
    return out


def assert_same(a, b):
    assert len(a["splits"]) == len(b["splits"])
    for x, y in zip(a["splits"], b["splits"]):
        assert np.array_equal(x, y)
    assert np.array_equal(a["rf_matrix"], b["rf_matrix"]) and np.array_equal(a["rf_to"], b["rf_to"])
    for key in ("fbp", "tbe"):
        assert np.array_equal(a[key][1], b[key][1])
        assert a[key][0].tobytes() == b[key][0].tobytes()


def assert_matches(got, want):
    for b, w in enumerate(got["splits"]):
        assert np.array_equal(w, want["splits"][b]), b
    assert np.array_equal(got["rf_matrix"], want["rf_matrix"])
    assert np.array_equal(got["rf_to"], want["rf_to"])
    for key in ("fbp", "tbe"):
        sums, support = want[key]
        assert got[key][1].tolist() == sums, key
        assert got[key][0].tobytes() == np.array(support, dtype=np.float64).tobytes(), key


CASES = [(4, 1, "random"), (4, 2, "random"), (5, 2, "random"), (33, 2, "random"), (64, 2, "random"), (68, 70, "random"),
         (130, 3, "random"), (200, 2, "caterpillar"), (256, 2, "balanced")]


@pytest.mark.parametrize("T,B,shape", CASES)
def test_against_the_restatement(product, T, B, shape):
    labels, ids, ref, trees = make_case(T, B, shape)
    got = results(product, labels, ref, trees)
    assert_matches(got, expected((T, B, shape), labels, ids, ref, trees))
    # the first tree is the reference: every split found, full support
    assert got["rf_to"][0] == 0 and got["rf_matrix"][0, 0] == 0


def test_fixture_trees(product):
    """the reference's recorded numbers, straight from the fixture"""
    with open(rs.FIXTURES) as f:
        cases = json.load(f)["cases"]
    for case in cases:
        T, labels = case["tips"], case["labels"]
        with pc.TreeSet(product, T, labels) as ts:
            for t in case["trees"]:
                assert ts.add(t), (product.errno, product.errmsg)
            for b in range(5):
                assert ts.splits(b).tolist() == case["splits"][b], (T, b)
            assert ts.rf_to(case["ref"]).tolist() == case["rf_to_ref"]
            assert ts.rf_matrix()[0].tolist() == case["rf_to_first"]
            support, sums = ts.support(case["ref"], pc.SUPPORT_TBE)
            assert np.allclose(support, np.mean(np.array(case["tbe"]), axis=0), rtol=0, atol=1e-15)
        for b in range(5):                                     # one tree at a time: the reference's values
            with pc.TreeSet(product, T, labels) as ts:
                assert ts.add(case["trees"][b])
                support, _ = ts.support(case["ref"], pc.SUPPORT_TBE)
                # values in [0, 1]: the reference rounds a quotient and a difference (2^-54 each at most), the set
                # form one quotient (2^-54)
                assert np.abs(support - np.array(case["tbe"][b])).max() <= 1.5 * 2.0 ** -53, (T, b)


@pytest.mark.parametrize("batch", ["1", "3"])
def test_batch_size_changes_nothing(product, monkeypatch, batch):
    labels, ids, ref, trees = make_case(68, 70, "random")
    want = expected((68, 70, "random"), labels, ids, ref, trees)
    monkeypatch.setenv("PLLHIP_TREESET_BATCH", batch)
    assert_matches(results(product, labels, ref, trees), want)


def test_hash_bits_change_nothing(product, monkeypatch):
    labels, ids, ref, trees = make_case(33, 7, "random", seed=5)
    plain = results(product, labels, ref, trees)
    assert_matches(plain, expected((33, 7, "random", 5), labels, ids, ref, trees))
    monkeypatch.setenv("PLLHIP_SPLIT_HASH_BITS", "0")
    blind = results(product, labels, ref, trees)
    assert_same(plain, blind)
    # without a hash every split walks one chain from slot 0 and is compared in full with what it meets
    distinct = len({tuple(w) for s in plain["splits"] for w in s.tolist()})
    assert blind["counts"][0] >= distinct * (distinct - 1) // 2 > plain["counts"][0]
    assert blind["counts"][1] > plain["counts"][1] >= 7 * 30 - distinct


def test_twice_the_same(product):
    labels, ids, ref, trees = make_case(130, 3, "random")
    with pc.TreeSet(product, 130, labels) as ts:
        for t in trees:
            assert ts.add(rs.to_newick(t))
        for kind in (pc.SUPPORT_FBP, pc.SUPPORT_TBE):
            a, b = ts.support(rs.to_newick(ref), kind), ts.support(rs.to_newick(ref), kind)
            assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
        assert np.array_equal(ts.rf_matrix(), ts.rf_matrix())
        assert np.array_equal(ts.splits(1), ts.splits(1))
    assert_same(results(product, labels, ref, trees), results(product, labels, ref, trees))


def test_trees_added_after_a_query(product):
    labels, ids, ref, trees = make_case(33, 7, "random", seed=5)
    want = expected((33, 7, "random", 5), labels, ids, ref, trees)
    with pc.TreeSet(product, 33, labels) as ts:
        for t in trees[:3]:
            assert ts.add(rs.to_newick(t))
        assert np.array_equal(ts.rf_matrix(), want["rf_matrix"][:3, :3])
        for t in trees[3:]:
            assert ts.add(rs.to_newick(t))
        assert np.array_equal(ts.rf_matrix(), want["rf_matrix"])
        assert ts.support(rs.to_newick(ref), pc.SUPPORT_TBE)[1].tolist() == want["tbe"][0]


def _parse(lib, newick):
    t = lib.lib.pll_utree_parse_newick_string(newick.encode())
    assert t, lib.errmsg
    return t


def test_labels_against_renumbered_node_indices(product):
    """a labelled set takes ids from labels whatever the trees' node_index says; an unlabelled set, fed the same
    trees renumbered so that node_index = index of the label, gives the same"""
    lib = product
    labels, ids, ref, trees = make_case(33, 4, "random", seed=9)
    parsed = [_parse(lib, rs.to_newick(t)) for t in trees + [ref]]
    numbering = [[p.contents.nodes[i].contents.node_index for i in range(33)] for p in parsed]
    by_label = [[p.contents.nodes[i].contents.label.decode() for i in range(33)] for p in parsed]
    assert any([ids[l] for l in names] != idx for names, idx in zip(by_label, numbering)), "numberings differ"
    out = []
    for renumber in (False, True):
        if renumber:
            for p in parsed:
                for i in range(33):
                    n = p.contents.nodes[i].contents
                    n.node_index = ids[n.label.decode()]
        with pc.TreeSet(lib, 33, None if renumber else labels) as ts:
            for p in parsed[:-1]:
                assert ts.add(p), (lib.errno, lib.errmsg)
            out.append(dict(splits=[ts.splits(b) for b in range(4)], rf_matrix=ts.rf_matrix(), rf_to=ts.rf_to(parsed[-1]),
                            fbp=ts.support(parsed[-1], pc.SUPPORT_FBP), tbe=ts.support(parsed[-1], pc.SUPPORT_TBE)))
    for p in parsed:
        lib.lib.pll_utree_destroy(p, None)
    assert_same(out[0], out[1])
    assert_matches(out[0], expected((33, 4, "random", 9), labels, ids, ref, trees))


def test_split_tbe_out(product):
    """the reference's own test: its printed values to the six decimals it prints, in the order its tip numbering
    gives, and a map from splits to edges of the caller's tree"""
    lib = product
    with open(rs.FIXTURES) as f:
        own = json.load(f)["split_tbe_out"]
    ids = rs.parsed_ids(lib, own["ref"])
    ref_tree = rs.parse_newick(own["ref"])
    want_splits = rs.splits(ref_tree, ids)
    for pair in own["pairs"]:
        ref, boot = _parse(lib, own["ref"]), _parse(lib, pair["tree"])
        for i in range(20):                                    # what pllmod_utree_consistency_set does
            n = boot.contents.nodes[i].contents
            n.node_index = ids[n.label.decode()]
        with pc.TreeSet(lib, 20) as ts:
            assert ts.add(boot), (lib.errno, lib.errmsg)
            support, sums, sides = ts.support(ref, pc.SUPPORT_TBE, with_map=True)
        assert " ".join("%.6f" % v for v in support) == pair["printed"]
        for split, side in zip(want_splits, sides):
            below = sum(1 << ids[l] for l in side)
            assert rs.normalise(below, 20) == split
        lib.lib.pll_utree_destroy(ref, None)
        lib.lib.pll_utree_destroy(boot, None)


def test_errors_leave_the_set_usable(product):
    lib = product
    labels, ids, ref, trees = make_case(33, 2, "random")
    want = expected((33, 2, "random"), labels, ids, ref, trees)
    with pc.TreeSet(lib, 33, labels) as ts:
        lib.errno = 0
        assert ts.rf_matrix() is None and lib.errno == pc.PLL_ERROR_PARAM_INVALID          # an empty set
        for t in trees:
            assert ts.add(rs.to_newick(t))
        assert np.array_equal(ts.rf_matrix(), want["rf_matrix"])
        wrong_label = rs.to_newick(ref).replace("x7,", "nobody,").replace("x7)", "nobody)")
        small = rs.to_newick(rs.random_tree(labels[:32], random.Random(2)))
        multi = "(" + ",".join(labels) + ");"
        for call, code in [(lambda: ts.splits(2), pc.PLL_ERROR_PARAM_INVALID),
                           (lambda: ts.support(rs.to_newick(ref), 7), pc.PLL_ERROR_PARAM_INVALID),
                           (lambda: ts.support(wrong_label, pc.SUPPORT_TBE), pc.PLL_ERROR_PARAM_INVALID),
                           (lambda: ts.rf_to(wrong_label), pc.PLL_ERROR_PARAM_INVALID),
                           (lambda: ts.rf_to(small), pc.PLL_ERROR_TREE_INVALID),
                           (lambda: ts.support(multi, pc.SUPPORT_FBP), pc.PLL_ERROR_TREE_INVALID),
                           (lambda: ts.add(multi) or None, pc.PLL_ERROR_TREE_INVALID)]:
            lib.errno = 0
            assert call() is None
            assert lib.errno == code, (lib.errno, lib.errmsg)
        assert lib.lib.pllhip_treeset_splits(ts.h, 0, None) == 0 and lib.errno == pc.PLL_ERROR_PARAM_INVALID
        assert lib.lib.pllhip_treeset_support(None, None, 0, None, None) == 0
        assert ts.count == 2
        assert_matches(dict(splits=[ts.splits(0), ts.splits(1)], rf_matrix=ts.rf_matrix(), rf_to=ts.rf_to(rs.to_newick(ref)),
                            fbp=ts.support(rs.to_newick(ref), pc.SUPPORT_FBP),
                            tbe=ts.support(rs.to_newick(ref), pc.SUPPORT_TBE)), want)
        up, kernel, down = ts.last_times()
        assert up >= 0 and kernel > 0 and down > 0
