"""Splits, RF distances, Felsenstein and transfer bootstrap support restated by brute force (sets of tips as Python
integers, O(T^3)), pinned to pll-modules by tests/golden/tree_support_fixtures.json (recorded by
tests/golden/record_tree_support.c: pllmod_utree_split_create, pllmod_utree_split_rf_distance, pllmod_utree_tbe_naive,
and the reference's own expected output test/out/tree/split-tbe.out), and the properties of the host flattener
(csrc/host/pllhip_treeset.c) through pllhip_treeset_add / pllhip_treeset_plan, which touch no device.

tests/test_tree_support_gpu.py checks the device against this file.

A tree here is a nested list: the top list has three entries, every other list two, a leaf is its label."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest

import pllhip_ctypes as pc

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_support_fixtures.json")


# --- trees ------------------------------------------------------------------------------------------------------

def parse_newick(text):
    """nested lists of labels; branch lengths and inner labels are dropped.  A top list of two entries whose one
    entry is a list is unrooted into three."""
    tokens = re.findall(r"[(),;]|[^(),;]+", text.strip())
    pos = 0

    def node():
        nonlocal pos
        if tokens[pos] == "(":
            pos += 1
            kids = [node()]
            while tokens[pos] == ",":
                pos += 1
                kids.append(node())
            assert tokens[pos] == ")", tokens[pos]
            pos += 1
            if pos < len(tokens) and tokens[pos] not in "(),;":
                pos += 1                                       # support value and length of an inner node
            return kids
        label = tokens[pos].split(":")[0].strip()
        pos += 1
        return label

    top = node()
    if len(top) == 2:
        a, b = top
        top = a + [b] if isinstance(a, list) else b + [a]
    return top


def to_newick(tree):
    def text(n):
        return n if isinstance(n, str) else "(" + ",".join(text(k) for k in n) + ")"
    return text(tree) + ";"


def leaves(node):
    return [node] if isinstance(node, str) else [l for k in node for l in leaves(k)]


def caterpillar(labels):
    tree = [labels[-2], labels[-1]]
    for l in reversed(labels[2:-2]):
        tree = [l, tree]
    return [labels[0], labels[1], tree]


def balanced(labels):
    def build(ls):
        return ls[0] if len(ls) == 1 else [build(ls[:len(ls) // 2]), build(ls[len(ls) // 2:])]
    third = len(labels) // 3
    return [build(labels[:third]), build(labels[third:2 * third]), build(labels[2 * third:])]


def _places(tree):
    """(parent list, index) of every node below the top"""
    out, stack = [], [tree]
    while stack:
        n = stack.pop()
        for i, k in enumerate(n):
            out.append((n, i))
            if isinstance(k, list):
                stack.append(k)
    return out


def random_tree(labels, rng):
    tree = list(labels[:3])
    for l in labels[3:]:
        parent, i = rng.choice(_places(tree))
        parent[i] = [parent[i], l]
    return tree


def copy_tree(tree):
    return [copy_tree(k) if isinstance(k, list) else k for k in tree]


def moved(tree, moves, rng):
    """a copy of `tree` with `moves` leaves pruned and regrafted somewhere else"""
    tree = copy_tree(tree)
    while moves:
        parent, i = rng.choice([(p, i) for p, i in _places(tree) if isinstance(p[i], str) and p is not tree])
        leaf, sibling = parent[i], parent[1 - i]
        grand = next((p, k) for p, k in _places(tree) if p[k] is parent)
        grand[0][grand[1]] = sibling
        target, k = rng.choice(_places(tree))
        target[k] = [target[k], leaf]
        moves -= 1
    return tree


# --- the definitions --------------------------------------------------------------------------------------------

def subtree_sets(tree, ids):
    """tips below every node under the top, tips included, as bit sets (bit id)"""
    out = []

    def below(n):
        s = 1 << ids[n] if isinstance(n, str) else 0
        if isinstance(n, list):
            for k in n:
                s |= below(k)
        out.append(s)
        return s

    for k in tree:
        below(k)
    return out


def normalise(s, T):
    return s if s & 1 else ((1 << T) - 1) & ~s


def words_of(s, T):
    return tuple((s >> (32 * w)) & 0xffffffff for w in range((T + 31) // 32))


def splits(tree, ids):
    """the T - 3 normalised splits as bit sets, ascending by words compared as unsigned, word 0 first"""
    T = len(ids)
    found = {normalise(s, T) for s in subtree_sets(tree, ids) if 1 < bin(s).count("1") < T - 1}
    assert len(found) == T - 3, "not a binary tree"
    return sorted(found, key=lambda s: words_of(s, T))


def split_words(tree, ids):
    T = len(ids)
    return np.array([words_of(s, T) for s in splits(tree, ids)], dtype=np.uint32).reshape(T - 3, (T + 31) // 32)


def rf(a, b, ids):
    return 2 * (len(ids) - 3 - len(set(splits(a, ids)) & set(splits(b, ids))))


def fbp_counts(ref, trees, ids):
    have = [set(splits(t, ids)) for t in trees]
    return [sum(s in h for h in have) for s in splits(ref, ids)]


def light_side(s, T):
    p = bin(s).count("1")
    return min(p, T - p)


def transfer_distances(ref, tree, ids):
    """delta of every reference split against one tree"""
    T = len(ids)
    nodes, have = subtree_sets(tree, ids), set(splits(tree, ids))
    out = []
    for r in splits(ref, ids):
        if r in have:
            out.append(0)
            continue
        best = light_side(r, T) - 1
        for s in nodes:
            d = bin(r ^ s).count("1")
            best = min(best, d, T - d)
        out.append(best)
    return out


def tbe_one_tree(ref, tree, ids):
    """1 - delta / (p - 1), as pllmod_utree_tbe_naive rounds it"""
    T = len(ids)
    return [1.0 - float(d) / (light_side(r, T) - 1)
            for r, d in zip(splits(ref, ids), transfer_distances(ref, tree, ids))]


def tbe_set(ref, trees, ids):
    """(sum of delta per split, support): the one division (B (p - 1) - sum) / (B (p - 1))"""
    T, B = len(ids), len(trees)
    sums = [sum(col) for col in zip(*[transfer_distances(ref, t, ids) for t in trees])]
    dens = [B * (light_side(r, T) - 1) for r in splits(ref, ids)]
    return sums, [(den - s) / den for s, den in zip(sums, dens)]


def fbp_set(ref, trees, ids):
    counts = fbp_counts(ref, trees, ids)
    return counts, [c / len(trees) for c in counts]


# --- the fixture ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixtures():
    with open(FIXTURES) as f:
        return json.load(f)


def test_fixture_cases_are_the_issue_s(fixtures):
    assert [c["tips"] for c in fixtures["cases"]] == [4, 5, 8, 31, 32, 33, 64, 65]
    assert all(len(c["trees"]) == 5 for c in fixtures["cases"])


def test_restatement_reproduces_the_reference(fixtures):
    for case in fixtures["cases"]:
        T = case["tips"]
        ids = {l: i for i, l in enumerate(case["labels"])}
        ref = parse_newick(case["ref"])
        trees = [parse_newick(t) for t in case["trees"]]
        assert sorted(leaves(ref)) == sorted(ids)
        assert split_words(ref, ids).tolist() == case["ref_splits"], T
        for b, tree in enumerate(trees):
            assert split_words(tree, ids).tolist() == case["splits"][b], (T, b)
            assert rf(trees[0], tree, ids) == case["rf_to_first"][b], (T, b)
            assert rf(ref, tree, ids) == case["rf_to_ref"][b], (T, b)
            got = np.array(tbe_one_tree(ref, tree, ids))
            assert got.tobytes() == np.array(case["tbe"][b], dtype=np.float64).tobytes(), (T, b)
        # an identical tree: every split found
        assert case["rf_to_ref"][0] == 0 and all(v == 1.0 for v in case["tbe"][0])


def parsed_ids(lib, newick):
    """label -> node_index as the library's Newick parser numbers the tips"""
    t = lib.lib.pll_utree_parse_newick_string(newick.encode())
    assert t, lib.errmsg
    ids = {t.contents.nodes[i].contents.label.decode(): t.contents.nodes[i].contents.node_index
           for i in range(t.contents.tip_count)}
    lib.lib.pll_utree_destroy(t, None)
    return ids


def test_restatement_reproduces_split_tbe_out(fixtures, product_nogpu):
    """the reference's own expected output: seventeen values per pair, in the split order that the parser's tip
    numbering of the reference tree gives"""
    own = fixtures["split_tbe_out"]
    ids = parsed_ids(product_nogpu, own["ref"])
    assert sorted(ids.values()) == list(range(20))
    ref = parse_newick(own["ref"])
    for pair in own["pairs"]:
        _, support = tbe_set(ref, [parse_newick(pair["tree"])], ids)
        assert " ".join("%.6f" % v for v in support) == pair["printed"]
        assert " ".join("%.6f" % v for v in tbe_one_tree(ref, parse_newick(pair["tree"]), ids)) == pair["printed"]


def test_set_support_is_the_mean_of_the_trees(fixtures):
    case = fixtures["cases"][5]
    ids = {l: i for i, l in enumerate(case["labels"])}
    ref, trees = parse_newick(case["ref"]), [parse_newick(t) for t in case["trees"]]
    _, support = tbe_set(ref, trees, ids)
    mean = np.mean(np.array(case["tbe"]), axis=0)
    assert np.allclose(support, mean, rtol=0, atol=1e-15)
    counts, fbp = fbp_set(ref, trees, ids)
    assert counts == [sum(row[i] == 1.0 for row in case["tbe"]) for i in range(len(counts))]
    assert fbp == [c / 5 for c in counts]


# --- the flattener ----------------------------------------------------------------------------------------------

def labels_for(T):
    return ["x%d" % i for i in range(T)]


def run_program(program, T):
    """walks a transfer program with sets: (tips below every combined node in program order, deepest stack)"""
    stack, nodes, deepest = [], [], 0
    for kind, arg in program:
        if kind == 0:
            stack.append(1 << int(arg))
        else:
            assert kind == 1 and len(stack) >= 2
            b, a = stack.pop(), stack.pop()
            assert a & b == 0
            stack.append(a | b)
            assert bin(a | b).count("1") == arg, "a combine step states the node's size"
            nodes.append(a | b)
        deepest = max(deepest, len(stack))
    assert len(stack) == 1 and stack[0] == ((1 << T) - 1) & ~1, "everything but tip 0 ends up in one entry"
    return nodes, deepest


def check_plan(lib, tree, labels):
    T = len(labels)
    ids = {l: i for i, l in enumerate(labels)}
    with pc.TreeSet(lib, T, labels) as ts:
        assert ts.add(to_newick(tree)), (lib.errno, lib.errmsg)
        assert ts.count == 1
        order, lo, hi, program, deepest = ts.plan(0)
    assert sorted(order.tolist()) == list(range(1, T)), "every tip but tip 0, once"
    assert len(program) == 2 * T - 3 and (program[:, 0] == 0).sum() == T - 1
    # every inner edge is an interval of the order, and none holds tip 0: the split is its complement
    want = set(splits(tree, ids))
    got = set()
    for a, b in zip(lo.tolist(), hi.tolist()):
        assert 0 <= a and a + 2 <= b <= T - 1
        below = sum(1 << int(t) for t in order[a:b])
        got.add(((1 << T) - 1) & ~below)
    assert got == want
    nodes, walked = run_program(program.tolist(), T)
    assert walked == deepest <= 1 + int(np.floor(np.log2(T)))
    assert {normalise(s, T) for s in nodes if bin(s).count("1") < T - 1} == want
    assert [int(t) for k, t in program.tolist() if k == 0] == order.tolist(), "pushes follow the tip order"
    return deepest


def test_flattener_stack_bound_on_a_caterpillar(product_nogpu):
    labels = labels_for(300)
    assert check_plan(product_nogpu, caterpillar(labels), labels) == 2
    rng = random.Random(3)
    shuffled = labels[:]
    rng.shuffle(shuffled)
    # tip 0 somewhere along the spine: two caterpillars hang below its neighbour
    assert check_plan(product_nogpu, caterpillar(shuffled), labels) <= 3


def test_flattener_stack_bound_on_a_balanced_tree(product_nogpu):
    labels = labels_for(256)
    assert check_plan(product_nogpu, balanced(labels), labels) <= 9


@pytest.mark.parametrize("T", [4, 5, 33, 68])
def test_flattener_intervals_on_random_trees(product_nogpu, T):
    rng = random.Random(T)
    labels = labels_for(T)
    for _ in range(3):
        check_plan(product_nogpu, random_tree(labels, rng), labels)


def test_flattener_leaves_the_tree_alone(product_nogpu):
    lib, labels = product_nogpu, labels_for(12)
    newick = to_newick(random_tree(labels, random.Random(1)))
    t = lib.lib.pll_utree_parse_newick_string(newick.encode())
    size = C.sizeof(pc.UNode)
    before = [C.string_at(C.addressof(t.contents.nodes[i].contents), size)
              for i in range(t.contents.tip_count + t.contents.inner_count)]
    with pc.TreeSet(lib, 12, labels) as ts:
        assert ts.add(t)
    after = [C.string_at(C.addressof(t.contents.nodes[i].contents), size)
             for i in range(t.contents.tip_count + t.contents.inner_count)]
    lib.lib.pll_utree_destroy(t, None)
    assert before == after


def test_flattener_rejections(product_nogpu):
    lib, labels = product_nogpu, labels_for(6)
    good = "((x0,x1),(x2,x3),(x4,x5));"
    with pc.TreeSet(lib, 6, labels) as ts:
        for newick, code in [("((x0,x1),(x2,x3),(x4,zz));", pc.PLL_ERROR_PARAM_INVALID),       # unknown label
                             ("((x0,x1),(x2,x3),(x4,x4));", pc.PLL_ERROR_PARAM_INVALID),       # duplicate, x5 missing
                             ("((x0,x1),(x2,x3),x4);", pc.PLL_ERROR_TREE_INVALID),             # five tips
                             ("((x0,x1),x2,x3,(x4,x5));", pc.PLL_ERROR_TREE_INVALID),          # four at the top
                             ("((x0,x1,x2),x3,(x4,x5));", pc.PLL_ERROR_TREE_INVALID)]:         # three below a node
            lib.errno = 0
            assert not ts.add(newick), newick
            assert lib.errno == code, (newick, lib.errno, lib.errmsg)
            assert ts.count == 0
        assert ts.add(good) and ts.count == 1
        assert ts.plan(1) is None and lib.errno == pc.PLL_ERROR_PARAM_INVALID
    # the label table
    for bad in (labels[:5] + ["x0"], labels[:5] + [None]):
        lib.errno = 0
        ts = pc.TreeSet(lib, 6, bad)
        assert not ts.h and lib.errno == pc.PLL_ERROR_PARAM_INVALID
    lib.errno = 0
    assert not pc.TreeSet(lib, 3, None).h and lib.errno == pc.PLL_ERROR_PARAM_INVALID
    assert not pc.TreeSet(lib, 65536, None).h


def test_flattener_tip_ids_without_labels(product_nogpu):
    lib = product_nogpu
    t = lib.lib.pll_utree_parse_newick_string(b"((a,b),(c,d),(e,f));")
    tips = [t.contents.nodes[i].contents for i in range(6)]
    assert sorted(n.node_index for n in tips) == list(range(6))
    with pc.TreeSet(lib, 6) as ts:
        assert ts.add(t)
        keep = tips[2].node_index
        for bad in (6, tips[3].node_index):                    # out of range; twice the same
            tips[2].node_index = bad
            lib.errno = 0
            assert not ts.add(t) and lib.errno == pc.PLL_ERROR_PARAM_INVALID, lib.errmsg
        tips[2].node_index = keep
        assert ts.add(t) and ts.count == 2
        order0, order1 = ts.plan(0)[0], ts.plan(1)[0]
        assert order0.tolist() == order1.tolist()
    lib.lib.pll_utree_destroy(t, None)


def test_a_query_without_a_device_is_an_error(product_nogpu):
    """no quiet fall-back: where no device is visible a query fails, and the set stays as it was"""
    lib = product_nogpu
    if lib.lib.pllhip_device_count() > 0:
        return
    with pc.TreeSet(lib, 6, labels_for(6)) as ts:
        assert ts.add("((x0,x1),(x2,x3),(x4,x5));")
        for call in (ts.rf_matrix, lambda: ts.splits(0), lambda: ts.rf_to("((x0,x1),(x2,x3),(x4,x5));"),
                     lambda: ts.support("((x0,x1),(x2,x3),(x4,x5));", pc.SUPPORT_TBE)):
            lib.errno = 0
            assert call() is None and lib.errno == pc.PLL_ERROR_HIP_NODEVICE, (lib.errno, lib.errmsg)
        assert ts.count == 1 and ts.add("((x0,x2),(x1,x3),(x4,x5));") and ts.count == 2
