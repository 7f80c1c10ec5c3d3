"""The consensus of a tree set (strict, majority rule, extended majority rule) restated by brute force, pinned to
pll-modules by tests/golden/consensus_fixtures.json (recorded by tests/golden/record_consensus.c from
pllmod_utree_weight_consensus with weights 1/B), and the host side of the feature (csrc/host/pllhip_consensus.c: the
integer thresholds and the tree of a split system), which touches no device.

tests/test_consensus_gpu.py checks the device against this file.

The contract (include/pllhip.h): with B trees and c the number of trees that hold a split, every split with
c >= need_major is in; for a threshold below 0.5 the splits with c >= need_minor are then gone through in rank order
(c descending, words ascending as unsigned, word 0 first) and each one compatible with everything held is taken, until
T - 3 are held.  Splits are sets of tips as Python integers, in normal form (tip 0's bit set)."""
import collections
import json
import os
import random
import re

import numpy as np
import pytest

import pllhip_ctypes as pc
import test_tree_support_restatement as rs

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consensus_fixtures.json")
THRESHOLDS = [1.0, 0.75, 0.5, 0.25, 0.0]


# --- the definitions --------------------------------------------------------------------------------------------

def needs(B, threshold):
    """(need_major, need_minor): the smallest counts that are "above max(threshold, 0.5)" and "above threshold"""
    assert 0.0 <= threshold <= 1.0 and B > 0
    if threshold == 1.0:
        major = B
    elif threshold <= 0.5:
        major = next(c for c in range(B + 1) if 2 * c > B)
    else:
        major = next(c for c in range(B + 1) if c / B > threshold)     # int / int: one correctly rounded quotient
    if threshold >= 0.5:
        minor = major
    else:
        minor = max(1, next(c for c in range(B + 1) if c / B > threshold))
    return major, minor


def compatible(a, b, T):
    """two splits in normal form: one holds the other, or together they hold every tip"""
    return a & ~b == 0 or b & ~a == 0 or a | b == (1 << T) - 1


def split_counts(trees, ids):
    return collections.Counter(s for t in trees for s in rs.splits(t, ids))


def ranked_candidates(counts, T, B, threshold):
    minor = needs(B, threshold)[1]
    return sorted(((s, c) for s, c in counts.items() if c >= minor), key=lambda sc: (-sc[1], rs.words_of(sc[0], T)))


def consensus(trees, ids, threshold, stats=None):
    """[(split, trees that hold it)] in rank order: the sequential definition"""
    T, B = len(ids), len(trees)
    major = needs(B, threshold)[0]
    ranked = ranked_candidates(split_counts(trees, ids), T, B, threshold)
    held = [sc for sc in ranked if sc[1] >= major]
    if threshold < 0.5:
        for s, c in ranked:
            if len(held) == T - 3:
                break
            if c < major and all(compatible(s, h, T) for h, _ in held):
                held.append((s, c))
    if stats is not None:
        stats["candidates"], stats["distinct"] = len(ranked), len(split_counts(trees, ids))
    return held


def tie_independent(trees, ids, threshold):
    """no run of equal counts among the candidates holds two incompatible splits: their order cannot matter"""
    T, B = len(ids), len(trees)
    runs = collections.defaultdict(list)
    for s, c in ranked_candidates(split_counts(trees, ids), T, B, threshold):
        runs[c].append(s)
    return all(compatible(a, b, T) for run in runs.values() for i, a in enumerate(run) for b in run[:i])


def words_array(held, T):
    return np.array([rs.words_of(s, T) for s, _ in held], dtype=np.uint32).reshape(len(held), (T + 31) // 32)


def from_words(rows):
    return [sum(int(w) << (32 * i) for i, w in enumerate(row)) for row in rows]


# --- the integer thresholds -------------------------------------------------------------------------------------

def test_needs_by_hand():
    assert needs(1, 1.0) == (1, 1) and needs(1, 0.0) == (1, 1)
    assert needs(2, 0.5) == (2, 2), "one tree of two is exactly half and no majority"
    assert needs(3, 0.5) == (2, 2) and needs(8, 0.5) == (5, 5) and needs(31, 0.5) == (16, 16)
    assert needs(8, 0.75) == (7, 7), "six of eight is not above three quarters"
    assert needs(8, 0.25) == (5, 3) and needs(16, 0.25) == (9, 5) and needs(31, 0.25) == (16, 8)
    assert needs(31, 0.0) == (16, 1) and needs(31, 1.0) == (31, 31)
    assert needs(10, 0.7) == (8, 8), "7 / 10 rounds to the double 0.7 and is not above it"
    assert needs(10, 0.3) == (6, 4), "3 / 10 rounds to the double 0.3 and is not above it"


def test_host_thresholds_follow_the_restatement(product_nogpu):
    lib = product_nogpu
    cuts = THRESHOLDS + [0.1, 0.2, 0.3, 0.4, 0.49999999999999994, 0.5000000000000001, 0.6, 0.7, 0.9, 0.9999999999999999,
                         1 / 3, 2 / 3, 5e-324]
    for B in list(range(1, 41)) + [70, 100, 999, 1000, 65535, 4000000000]:
        for cut in cuts:
            if B > 1000:
                major, minor = pc.consensus_needs(lib, B, cut)
                top = max(cut, 0.5)
                assert 1 <= minor <= major <= B
                assert (major == B) if cut == 1.0 else (major / B > top and (major - 1) / B <= top)
                assert minor == major if cut >= 0.5 else (minor / B > cut and (minor == 1 or (minor - 1) / B <= cut))
            else:
                assert pc.consensus_needs(lib, B, cut) == needs(B, cut), (B, cut)
    for bad in (-1e-300, 1.0000000000000002, float("nan"), float("inf"), -1.0, 2.0):
        lib.errno = 0
        assert pc.consensus_needs(lib, 5, bad) is None and lib.errno == pc.PLL_ERROR_PARAM_INVALID, bad
    lib.errno = 0
    assert pc.consensus_needs(lib, 0, 0.5) is None and lib.errno == pc.PLL_ERROR_PARAM_INVALID


# --- the fixture ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases():
    with open(FIXTURES) as f:
        out = json.load(f)["cases"]
    for case in out:
        case["ids"] = {l: i for i, l in enumerate(case["labels"])}
        case["parsed"] = [rs.parse_newick(t) for t in case["trees"]]
    return out


def test_fixture_cases_are_the_issue_s(cases):
    scrambled = [(c["tips"], len(c["trees"])) for c in cases if c["kind"] == "scramble"]
    assert scrambled == [(T, B) for T in (5, 8, 33, 40) for B in (1, 3, 5, 8, 16, 31)]
    assert sum(c["kind"] == "independent" for c in cases) == 1
    for c in cases:
        assert [r["threshold"] for r in c["results"]] == THRESHOLDS
        assert sorted(rs.leaves(c["parsed"][0])) == sorted(c["labels"])


def check_supports(case, result, counts):
    """the reference sums c copies of fl(1/B), the contract divides once: each of the c - 1 additions and the
    rounding of 1/B is off by at most 2^-53 relative, as is the one division"""
    B = len(case["trees"])
    for s, got in zip(from_words(result["splits"]), result["support"]):
        c = counts[s]
        assert abs(got - c / B) <= (c + 1) * 2.0 ** -53 * (c / B), (case["tips"], B, result["threshold"], c, got)


def test_restatement_reproduces_the_reference(cases):
    below, independent = 0, 0
    for case in cases:
        T, B, ids, trees = case["tips"], len(case["trees"]), case["ids"], case["parsed"]
        counts = split_counts(trees, ids)
        for result in case["results"]:
            cut, where = result["threshold"], (case["kind"], T, B, result["threshold"])
            theirs = from_words(result["splits"])
            assert len(set(theirs)) == len(theirs) and all(s & 1 and s in counts for s in theirs), where
            check_supports(case, result, counts)
            ours = consensus(trees, ids, cut)
            assert [c for _, c in ours] == sorted((c for _, c in ours), reverse=True), "rank order"
            major, minor = needs(B, cut)
            if cut >= 0.5:
                assert set(theirs) == {s for s, _ in ours} == {s for s, c in counts.items() if c >= major}, where
                continue
            below += 1
            if tie_independent(trees, ids, cut):
                independent += 1
                assert set(theirs) == {s for s, _ in ours}, where
                continue
            # what holds under any order of ties
            for held in (theirs, [s for s, _ in ours]):
                assert {s for s, c in counts.items() if c >= major} <= set(held), where
                assert all(counts[s] >= minor for s in held), where
                assert all(compatible(a, b, T) for i, a in enumerate(held) for b in held[:i]), where
                assert len(held) == T - 3 or not any(
                    all(compatible(s, h, T) for h in held) for s, c in counts.items() if c >= minor and s not in held), where
    assert below == 2 * len(cases)
    assert 2 * independent >= below, (independent, below)


def test_single_tree_and_equal_trees(cases):
    case = next(c for c in cases if c["tips"] == 33 and len(c["trees"]) == 1)
    for cut in THRESHOLDS:
        held = consensus(case["parsed"], case["ids"], cut)
        assert [s for s, _ in held] == rs.splits(case["parsed"][0], case["ids"]), "one tree: itself, ascending"
        assert consensus(case["parsed"] * 4, case["ids"], cut) == [(s, 4) for s, _ in held]


def test_two_different_trees(cases):
    """c = 1 of B = 2 is exactly half: no majority, and a candidate only below 0.5"""
    case = next(c for c in cases if c["tips"] == 8 and len(c["trees"]) == 5)
    ids = case["ids"]
    a = case["parsed"][0]
    b = next(t for t in case["parsed"] if set(rs.splits(t, ids)) != set(rs.splits(a, ids)))
    common = set(rs.splits(a, ids)) & set(rs.splits(b, ids))
    for cut in (1.0, 0.75, 0.5):
        assert {s for s, _ in consensus([a, b], ids, cut)} == common
    held = consensus([a, b], ids, 0.0)
    assert len(held) == 5 and common == {s for s, c in held if c == 2}


# --- the tree of a split system ---------------------------------------------------------------------------------

def tree_splits(newick, ids):
    """the non-trivial splits of a possibly multifurcating Newick tree, and the inner labels as doubles"""
    T = len(ids)
    tree = rs.parse_newick(newick)
    assert sorted(rs.leaves(tree)) == sorted(ids), "every tip once"
    found = [rs.normalise(s, T) for s in rs.subtree_sets(tree, ids) if 1 < bin(s).count("1") < T - 1]
    assert len(found) == len(set(found))
    return set(found), sorted(float(x) for x in re.findall(r"\)([0-9.eE+-]+):", newick))


def test_tree_of_a_split_system(product_nogpu, cases):
    lib = product_nogpu
    for case in cases:
        T, B, ids = case["tips"], len(case["trees"]), case["ids"]
        if B not in (1, 5, 31):
            continue
        for cut in THRESHOLDS:
            held = consensus(case["parsed"], ids, cut)
            support = [c / B for _, c in held]
            with pc.TreeSet(lib, T, case["labels"]) as ts:
                newick = ts.newick_from_splits(words_array(held, T), support)
                bare = ts.newick_from_splits(words_array(held, T))
            assert newick and bare, (lib.errno, lib.errmsg)
            got, labels = tree_splits(newick, ids)
            assert got == {s for s, _ in held}, (T, B, cut)
            assert labels == sorted(support), "the shortest decimal reads back as the same double"
            assert tree_splits(bare, ids) == (got, [])
            # the library's own parser takes it, tips and inner nodes counted
            t = lib.lib.pll_utree_parse_newick_string(newick.encode())
            assert t, lib.errmsg
            assert (t.contents.tip_count, t.contents.inner_count) == (T, len(held) + 1)
            lib.lib.pll_utree_destroy(t, None)


def test_tree_records(product_nogpu):
    """tips carry node_index = tip id and the set's labels; an unlabelled set gives no labels; K = 0 is the star"""
    lib, T = product_nogpu, 6
    labels = ["f", "e", "d", "c", "b", "a"]
    ids = {l: i for i, l in enumerate(labels)}
    held = [(s, 1) for s in rs.splits(rs.parse_newick("((f,e),(d,c),(b,a));"), ids)]
    words = words_array(held, T)
    for named in (True, False):
        with pc.TreeSet(lib, T, labels if named else None) as ts:
            tree = lib.lib.pllhip_treeset_tree_from_splits(ts.h, 3, words.ctypes.data_as(pc.c_uint_p), None)
            assert tree, lib.errmsg
            t = tree.contents
            assert (t.tip_count, t.inner_count, t.edge_count, t.binary) == (6, 4, 9, 1)
            for i in range(6):
                n = t.nodes[i].contents
                assert n.node_index == i and n.clv_index == i and not n.next
                assert (n.label.decode() if n.label else None) == (labels[i] if named else None)
            assert t.vroot.contents.next and not t.nodes[0].contents.back.contents.back.contents.next
            lib.lib.pll_utree_destroy(tree, None)
            assert ts.newick_from_splits(words[:0]).count("(") == 1, "the star"


def test_tree_builder_rejections(product_nogpu):
    lib, T = product_nogpu, 8
    full = (1 << T) - 1
    good = [0b00000111, 0b00011111]
    with pc.TreeSet(lib, T) as ts:
        assert ts.newick_from_splits(np.array(good, np.uint32))
        for bad in ([0b00000111, 0b00000111],            # twice
                    [0b00000111, 0b00011101],            # neither nested nor disjoint nor covering
                    [0b00000110],                        # not in normal form
                    [0b00000001], [full & ~2], [full],   # trivial
                    [0b100000111]):                      # a bit beyond the tips
            lib.errno = 0
            assert ts.newick_from_splits(np.array(bad, np.uint32)) is None, bad
            assert lib.errno == pc.PLL_ERROR_PARAM_INVALID, (bad, lib.errno, lib.errmsg)
        lib.errno = 0
        assert not lib.lib.pllhip_treeset_tree_from_splits(ts.h, 6, np.zeros(6, np.uint32).ctypes.data_as(pc.c_uint_p), None)
        assert lib.errno == pc.PLL_ERROR_PARAM_INVALID, "more than T - 3 splits"
        assert not lib.lib.pllhip_treeset_tree_from_splits(None, 0, None, None)


def test_a_consensus_without_a_device_is_an_error(product_nogpu):
    """no quiet fall-back: the selection runs on the device or not at all; bad arguments are reported first"""
    lib = product_nogpu
    with pc.TreeSet(lib, 6, rs.labels_for(6)) as ts:
        lib.errno = 0
        assert ts.consensus(0.5) is None and lib.errno == pc.PLL_ERROR_PARAM_INVALID, "an empty set"
        assert ts.add("((x0,x1),(x2,x3),(x4,x5));")
        for bad in (-0.1, 1.5, float("nan")):
            lib.errno = 0
            assert ts.consensus(bad) is None and ts.consensus_newick(bad) is None
            assert lib.errno == pc.PLL_ERROR_PARAM_INVALID
        if lib.lib.pllhip_device_count() > 0:
            return
        for call in (lambda: ts.consensus(0.5), lambda: ts.consensus_newick(0.0)):
            lib.errno = 0
            assert call() is None and lib.errno == pc.PLL_ERROR_HIP_NODEVICE, (lib.errno, lib.errmsg)
        assert ts.count == 1 and ts.add("((x0,x2),(x1,x3),(x4,x5));") and ts.count == 2
