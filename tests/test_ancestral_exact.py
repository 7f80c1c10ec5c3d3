"""The ancestral-state kernels (kernels_ancestral.hpp, pllhip_node_ancestral_batch) and the per-call form
(pll_compute_node_ancestral, k_node_ancestral) against tests/ancestral_reference.py: the table of a triple in
numpy.longdouble from the vectors, the P-matrix, the frequencies and the weights the engine itself holds, under the
bound derived there, |got - ref| <= 2 (R S + S + 8) 2^-53 ref + 2^-1000 per entry.

The summary is checked twice: exactly against the engine's own table (states == argmax with the first index on
ties, state_probs == max), and against the reference on every row whose two largest reference values are further
apart than their bounds.  Rows the reference leaves all zero (a zero-length matrix between two tips whose states
differ) are not excluded: they must be all zero, with state 0 and probability 0.  The reference alone may exclude
at most 1 % of the remaining rows of a test.

CPU tests (no mark) validate the reference: against a brute-force enumeration of the inner states of a 5-tip tree,
and against the oracle's pll_compute_node_ancestral, which sums serially in fp64 and so falls under the same bound."""
import itertools

import numpy as np
import pytest

import ancestral_reference as ar
import pllhip_ctypes as pc

PROBS = pc.PLLHIP_ANC_PROBS
LD = np.longdouble
SITES = [1, 2, 31, 32, 33, 34, 64, 127, 128, 130]   # even and odd tails, full blocks, four full waves, a second workgroup

# (states, rate_cats): the kernel that has to run it
KERNELS = {
    (4, 4): "k_anc_s4", (4, 1): "k_anc_s4",
    (4, 3): "k_anc_s16<1>", (2, 4): "k_anc_s16<1>",
    (5, 4): "k_anc_s16<2>",
    (10, 4): "k_anc_s16<3>",
    (16, 4): "k_anc_s16<4>",
    (20, 12): "k_anc_s16<5>",                      # dynamic LDS above 64 KiB with the table, below without
    (24, 4): "k_anc_s16<6>",
    (28, 2): "k_anc_s16<7>",
    (32, 4): "k_anc_s16<8>", (32, 9): "k_anc_s16<8>",
    (20, 4): "k_anc_s20", (20, 1): "k_anc_s20", (20, 8): "k_anc_s20",
    (61, 4): "k_anc_generic, blocked rows", (48, 2): "k_anc_generic, blocked rows", (64, 1): "k_anc_generic, blocked rows",
    (20, 16): "k_anc_generic, API layout",
}
SHAPES = list(KERNELS)


def kernel_of(inst):
    """the ancestral kernel of a partition, from the family the engine reports (anc_stage_add dispatches on it)"""
    name = inst.L.pllhip_partials_kernel_name(inst.p)
    return {b"s4-valu": "k_anc_s4", b"s20-mfma": "k_anc_s20", b"s16-mfma": f"k_anc_s16<{(inst.S + 3) // 4}>",
            b"s61-mfma": "k_anc_generic, blocked rows", b"generic": "k_anc_generic, API layout"}[name]


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def pendant(tree, tip):
    (_, k), = tree.adj[tip]
    return k


def special_tree(ntips):
    """pc.Tree(ntips, 42, 43) with three branch lengths replaced: 0 on the pendant edge of tip `ta`, 1e-6 on that
    of tip `tb`, 50 on the first edge between two inner nodes that is not the (inner, inner) edge of the triples"""
    t = pc.Tree(ntips, 42, 43)
    tips = [x for x in range(ntips) if x != t.root_b]
    t.ta, t.tb = tips[0], tips[1]
    t.m_zero, t.m_short = pendant(t, t.ta), pendant(t, t.tb)
    # the (inner, inner) edge: an operation with an inner child, the one closest to the root edge
    t.parent, t.child, t.m_inner = next((op[0], c, m) for op in reversed(t.ops) for c, m in ((op[2], op[3]), (op[5], op[6]))
                                        if c >= ntips)
    t.m_long = next(k for k, (u, v) in enumerate(t.edges) if u >= ntips and v >= ntips and k != t.m_inner)
    t.brlens[t.m_zero], t.brlens[t.m_short], t.brlens[t.m_long] = 0.0, 1e-6, 50.0
    t.far = t.ops[0][0]                       # the first inner node of the post-order
    return t


def triples_of(t):
    """all four operand kinds, adjacent and not, with matrices that belong to the pair and matrices that do not"""
    out = [(t.parent, t.child, t.m_inner), (t.child, t.parent, t.m_inner),       # (inner, inner), a non-root edge
           (t.root_a, t.root_b, t.root_matrix),                                   # (inner, tip), the root edge
           (t.root_b, t.root_a, t.root_matrix),                                   # (tip, inner)
           (t.ta, t.tb, t.m_zero),                                                # (tip, tip), length 0
           (t.tb, t.ta, t.m_long),                                                # (tip, tip), length 50
           (t.far, t.ta, t.m_long)]                                               # (inner, tip), not adjacent
    if t.far != t.root_a:
        out.append((t.root_a, t.far, t.m_short))                                  # (inner, inner), not adjacent, 1e-6
    return out


def ambiguity_map(states):
    """'-' for every state and two partial codes: tests/_lookup_worker.py's B and Z at 20 states, R and Y at 4"""
    cmap = pc.state_charmap(states)
    if states == 4:
        cmap[ord("R")], cmap[ord("Y")] = 0b0101, 0b1010
        return cmap, "RY"
    cmap[ord("B")] = (1 << 2) | (1 << 3)
    cmap[ord("Z")] = (1 << (states - 3)) | (1 << (states - 2))
    return cmap, "BZ"


def build_case(lib, states, rate_cats, nsites, coded, inputs="plain", ntips=None, tree=None, **kw):
    """inputs: 'plain' (one model, equal weights, unambiguous states), 'mixture' (params_indices 0, 1, 0, 1, ... and
    unequal rate weights) or 'ambiguous' (gaps and two partial codes at every tip, the mixture as well)"""
    if tree is None:
        tree = special_tree(ntips or 9 + (states + rate_cats + nsites) % 4)
    codes = pc.random_codes(tree.ntips, nsites, states, 44)
    if hasattr(tree, "ta"):
        codes[tree.tb, ::3] = codes[tree.ta, ::3]           # the two tips of the zero-length matrix agree at every third site
    mixed = inputs != "plain" and rate_cats > 1
    inst = pc.build_instance(lib, states=states, rate_cats=rate_cats, ntips=tree.ntips, nsites=nsites, coded=coded,
                             tree=tree, codes=codes, mixture=[r % 2 for r in range(rate_cats)] if mixed else None, **kw)
    if mixed:
        w = pc._f64(np.arange(1.0, rate_cats + 1.0) / (rate_cats * (rate_cats + 1) / 2))
        inst.L.pll_set_category_weights(inst.p, w.ctypes.data_as(pc.c_double_p))
    if inputs == "ambiguous":
        assert states >= 4
        cmap, (c1, c2) = ambiguity_map(states)
        rnd = pc.splitmix64(49, tree.ntips * nsites).reshape(tree.ntips, nsites)
        for t in range(tree.ntips):
            seq = (codes[t] + 48).astype(np.uint8)
            seq[rnd[t] % np.uint64(5) == 0] = ord("-")
            seq[rnd[t] % np.uint64(7) == 1] = ord(c1)
            seq[rnd[t] % np.uint64(11) == 2] = ord(c2)
            if nsites >= 130 and hasattr(tree, "ta") and t in (tree.ta, tree.tb, tree.root_b):
                assert all((seq == ord(c)).any() for c in ("-", c1, c2))     # on the `node` and on the `other` side
            inst.set_tip_states(t, cmap, seq.tobytes())
    pc.full_traversal(inst)
    return inst


class Tally:
    """what a test saw: the worst error as a fraction of the bound, and the rows the reference excludes"""

    def __init__(self):
        self.worst, self.rows, self.excluded, self.zero = 0.0, 0, 0, 0

    def check(self, inst, ref, got, states=None, state_probs=None, where=""):
        R, S = inst.R, inst.S
        frac = ar.worst_fraction(got, ref, R, S)
        self.worst = max(self.worst, frac)
        assert frac <= 1.0, f"{where}: |got - ref| is {frac:.3g} of the bound"
        clear, zero = ar.clear_rows(ref, R, S)
        self.rows += int((~zero).sum())
        self.zero += int(zero.sum())
        self.excluded += int((~clear & ~zero).sum())
        assert not got[zero].any(), where
        if states is not None:
            # exactly, against the engine's own table ...
            assert np.array_equal(states, np.argmax(got, axis=1).astype(np.uint8)), where
            assert np.array_equal(state_probs, got.max(axis=1)), where
            # ... and against the reference wherever it decides
            assert np.array_equal(states[clear], np.argmax(ref, axis=1).astype(np.uint8)[clear]), where
            assert not states[zero].any() and not state_probs[zero].any(), where

    def close(self, label):
        print(f"ancestral-exact {label}: worst |got - ref| = {self.worst:.4f} of the bound; {self.rows} rows, "
              f"{self.excluded} excluded, {self.zero} all zero")
        assert self.excluded * 100 <= self.rows, (self.excluded, self.rows)


def references(inst, triples):
    return [ar.reference(inst, *t) for t in triples]


def run_batch(inst, triples):
    """the batch with the table and without: canaries intact, the two summaries bit-equal"""
    nodes, others, mats = zip(*triples)
    st, sp, pr, intact = inst.node_ancestral_batch(nodes, others, mats, PROBS, pad=8)
    assert intact
    st0, sp0, none, intact0 = inst.node_ancestral_batch(nodes, others, mats, 0, pad=8)
    assert intact0 and none is None
    assert np.array_equal(st0, st) and np.array_equal(sp0, sp)
    return st, sp, pr


def check_batch(inst, triples, tally, where, refs=None):
    st, sp, pr = run_batch(inst, triples)
    refs = refs or references(inst, triples)
    for k, ref in enumerate(refs):
        tally.check(inst, ref, pr[k], st[k], sp[k], where=f"{where} entry {k} {triples[k]}")
    return st, sp, pr


def per_call(inst, triple):
    node, other, m = triple
    t = inst.tree
    return inst.node_ancestral(node, t.scaler_of(node), other, t.scaler_of(other), m)


# ---------------------------------------------------------------------------
# CPU: the reference itself
# ---------------------------------------------------------------------------
def test_reference_against_brute_force(oracle):
    """the 5-tip setup of tests/test_ancestral.py::test_brute_force_posteriors (4 states, 2 rate categories, 3 sites,
    a partial ambiguity code and a gap): with the vectors oriented towards the root edge, the table of
    (root_a, root_b, root_matrix) is the posterior of the inner node root_a -- here from all 4^3 assignments of the
    three inner nodes, the joint probability written out edge by edge in longdouble"""
    ntips, S, R = 5, 4, 2
    seqs = ["0R2", "12-", "301", "0R3", "210"]
    t = pc.Tree(ntips, 7, 8)
    with pc.Instance(oracle, ntips, S, 3, R, attributes=pc.PLL_ATTRIB_PATTERN_TIP) as inst:
        inst.set_model(pc.DNA_GTR_RATES, pc.DNA_FREQS, oracle.gamma_cats(0.7, R))
        cmap = pc.state_charmap(S)
        cmap[ord("R")] = np.uint64(0b0101)
        for k in range(ntips):
            inst.set_tip_states(k, cmap, seqs[k].encode())
        inst.tree = t
        pc.full_traversal(inst)
        P = [np.asarray(inst.get_pmatrix(m), dtype=LD) for m in range(t.nedges)]
        pi, w = np.asarray(pc.DNA_FREQS, dtype=LD), np.full(R, LD(1) / R)
        inner = list(range(ntips, 2 * ntips - 2))
        assert len(inner) == 3 and t.root_a in inner and t.root_b < ntips
        want = np.zeros((3, S), dtype=LD)
        for site in range(3):
            mask = [int(cmap[ord(s[site])]) for s in seqs]
            for r in range(R):
                for assign in itertools.product(range(S), repeat=3):
                    x = dict(zip(inner, assign))
                    joint = pi[x[t.root_a]]
                    # every edge once, read from its inner end (reversibility: pi_i P_ij = pi_j P_ji makes the joint
                    # probability independent of the orientation of the inner edges as long as they point away from
                    # the node whose frequency starts the product)
                    for m, (u, v) in enumerate(t.edges):
                        if u < ntips or v < ntips:
                            tip, nd = (u, v) if u < ntips else (v, u)
                            joint = joint * sum(P[m][r, x[nd], j] for j in range(S) if (mask[tip] >> j) & 1)
                        else:
                            a, b = (u, v) if towards(t, t.root_a, u) < towards(t, t.root_a, v) else (v, u)
                            joint = joint * P[m][r, x[a], x[b]]
                    want[site, x[t.root_a]] += w[r] * joint
        want /= want.sum(axis=1, keepdims=True)
        ref = ar.reference(inst, t.root_a, t.root_b, t.root_matrix)
        assert ref.dtype == LD and ref.shape == (3, S)
        # the reference starts from the oracle's fp64 vectors of the two inner nodes below root_a: two levels of
        # (sum of 4 products) x (sum of 4 products), some 8 roundings each, against none in the enumeration
        assert np.all(np.abs(ref - want) <= 64 * LD(2.0) ** -53 * want)
        # and the oracle's own call sits within the derived bound of the reference
        got = per_call(inst, (t.root_a, t.root_b, t.root_matrix))
        assert ar.worst_fraction(got, ref, R, S) <= 1.0


def towards(t, start, node):
    """number of edges between two nodes of a pc.Tree"""
    seen, layer, d = {start}, [start], 0
    while node not in seen:
        layer = [v for u in layer for v, _ in t.adj[u] if v not in seen]
        seen.update(layer)
        d += 1
    return d if node != start else 0


ORACLE_CASES = [(4, 4, "plain"), (4, 4, "mixture"), (4, 4, "ambiguous"), (20, 4, "plain"), (20, 4, "mixture"),
                (20, 4, "ambiguous"), (61, 4, "plain"), (61, 2, "mixture"), (61, 4, "ambiguous"), (10, 3, "ambiguous")]


@pytest.mark.parametrize("coded", [True, False], ids=["coded", "tip-vectors"])
@pytest.mark.parametrize("states,rate_cats,inputs", ORACLE_CASES)
def test_reference_against_the_oracle(oracle, states, rate_cats, inputs, coded):
    """the oracle's pll_compute_node_ancestral on the oracle's own vectors and matrices: a serial fp64 sum of the same
    non-negative terms, so the derived bound applies to it.  The triples hold the zero-length matrix between two tips
    (all-zero rows where their states differ, a single 1 where they agree)."""
    tally = Tally()
    for nsites in (33, 130):
        with build_case(oracle, states, rate_cats, nsites, coded, inputs) as inst:
            triples = triples_of(inst.tree)
            for k, triple in enumerate(triples):
                ref = ar.reference(inst, *triple)
                tally.check(inst, ref, per_call(inst, triple), where=f"N={nsites} entry {k} {triple}")
                if triple[2] == inst.tree.m_zero and inputs == "plain":
                    same = inst.codes[inst.tree.ta] == inst.codes[inst.tree.tb]
                    assert same.any() and not same.all()
                    assert not ref[~same].any() and np.array_equal(ref[same].sum(axis=1), np.ones(same.sum()))
                    assert np.array_equal(ref[same].max(axis=1), np.ones(same.sum()))
    tally.close(f"oracle S={states} R={rate_cats} {inputs} coded={coded}")
    assert tally.zero > 0


def test_reference_excludes_few_rows_at_every_shape(oracle):
    """the 1 % cap of the GPU tests, on the oracle's data: per shape of the kernel table, with the inputs of the GPU
    tests, the rows whose two largest reference values lie within their bounds of each other"""
    for states, rate_cats in SHAPES:
        for inputs in ("plain", "ambiguous" if states >= 4 else "mixture"):
            rows = excluded = 0
            for nsites in (33, 130):
                with build_case(oracle, states, rate_cats, nsites, True, inputs) as inst:
                    for triple in triples_of(inst.tree):
                        clear, zero = ar.clear_rows(ar.reference(inst, *triple), rate_cats, states)
                        rows += int((~zero).sum())
                        excluded += int((~clear & ~zero).sum())
            assert excluded * 100 <= rows, (states, rate_cats, inputs, excluded, rows)


# ---------------------------------------------------------------------------
# GPU: every kernel of the table, every site count
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("coded", [True, False], ids=["coded", "tip-vectors"])
@pytest.mark.parametrize("states,rate_cats", SHAPES)
def test_batch_against_the_reference(product, states, rate_cats, coded):
    tally = Tally()
    for nsites in SITES:
        with build_case(product, states, rate_cats, nsites, coded) as inst:
            assert kernel_of(inst) == KERNELS[states, rate_cats]
            check_batch(inst, triples_of(inst.tree), tally, f"N={nsites}")
    tally.close(f"S={states} R={rate_cats} coded={coded} plain")
    assert tally.zero > 0                       # the zero-length matrix between two tips that differ


# a mixture needs two rate categories, a partial code four states
MIXED = [(S, R, inputs) for S, R in SHAPES for inputs in ("mixture", "ambiguous")
         if (R > 1 if inputs == "mixture" else S >= 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("coded", [True, False], ids=["coded", "tip-vectors"])
@pytest.mark.parametrize("states,rate_cats,inputs", MIXED)
def test_batch_with_a_mixture_and_with_ambiguity_codes(product, states, rate_cats, inputs, coded):
    """params_indices 0, 1, 0, 1 with unequal rate weights; with 'ambiguous', gaps and two partial codes at every tip
    as well, so on the `node` and on the `other` side of the tip triples"""
    tally = Tally()
    for nsites in (33, 130):
        with build_case(product, states, rate_cats, nsites, coded, inputs) as inst:
            assert kernel_of(inst) == KERNELS[states, rate_cats]
            if rate_cats > 1:
                freqs, weights = ar.model_of(inst)
                assert (freqs[0] != freqs[1]).any() and weights[0] != weights[1]
            check_batch(inst, triples_of(inst.tree), tally, f"N={nsites}")
    tally.close(f"S={states} R={rate_cats} coded={coded} {inputs}")


DEEP = [(4, 600, 4), (20, 260, 4), (61, 130, 4)]                   # tests/test_gpu_parity.py, deep-tree scaling
DEEP_RATE_SCALERS = [(4, 400, 4), (20, 200, 4), (61, 100, 4), (7, 250, 3), (2, 500, 4), (16, 200, 2), (10, 220, 4),
                     (20, 200, 3), (61, 100, 1), (33, 120, 2)]     # ... and test_per_rate_scalers


def deep_case(product, states, ntips, rate_cats, **kw):
    tally = Tally()
    tree = pc.Tree(ntips, 42, 43)
    with build_case(product, states, rate_cats, 65, True, tree=tree, **kw) as inst:
        top = tree.ops[-1]
        assert top[0] == tree.root_a
        # (the inner child with the most scaler counts)
        _, child, m = max((int(inst.get_scaler(tree.scaler_of(c)).sum()), c, k)
                          for c, k in ((top[2], top[3]), (top[5], top[6])) if c >= ntips)
        assert inst.get_scaler(tree.scaler_of(tree.root_a)).any(), "the vector carries no scaler count: not a deep tree"
        triples = [(tree.root_a, child, m), (child, tree.root_a, m), (tree.root_a, tree.root_b, tree.root_matrix),
                   (tree.root_b, tree.root_a, tree.root_matrix)]
        check_batch(inst, triples, tally, f"{ntips} tips")
    tally.close(f"S={states} R={rate_cats} deep tree of {ntips} tips {sorted(kw)}")


@pytest.mark.gpu
@pytest.mark.parametrize("states,ntips,rate_cats", DEEP)
def test_scaled_vectors(product, states, ntips, rate_cats):
    """a deep tree whose inner vectors carry scaler counts: the counts are ignored, the scaled doubles are the input"""
    deep_case(product, states, ntips, rate_cats)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ntips,rate_cats", DEEP_RATE_SCALERS)
def test_scaled_vectors_with_per_rate_scalers(product, states, ntips, rate_cats):
    deep_case(product, states, ntips, rate_cats, alpha=0.3 if states <= 20 else 1.0, attributes=pc.PLL_ATTRIB_RATE_SCALERS)


@pytest.mark.gpu
def test_ascertainment_partition(product):
    """PLL_ATTRIB_AB_LEWIS: the partition's arrays hold 4 constant patterns behind the 33 sites; exactly 33 rows are
    written and the canaries behind them survive (run_batch)"""
    tally = Tally()
    with build_case(product, 4, 4, 33, True, attributes=pc.PLL_ATTRIB_AB_FLAG | pc.PLL_ATTRIB_AB_LEWIS) as inst:
        inst.set_asc(pc.PLL_ATTRIB_AB_LEWIS)
        pc.full_traversal(inst)
        assert inst.Nalloc == 37 and inst.N == 33
        st, sp, pr = check_batch(inst, triples_of(inst.tree), tally, "asc")
        assert pr.shape[1:] == (33, 4)
    tally.close("S=4 R=4 ascertainment")


@pytest.mark.gpu
def test_partition_on_two_shards(product):
    """161 sites at 20 states over two shards (96 + 65 sites): the bits of the unsharded run, within the bound"""
    L = product.lib
    tally = Tally()
    with build_case(product, 20, 4, 161, True, "ambiguous") as plain:
        assert L.pllhip_set_sharding(2, None)
        try:
            shard = build_case(product, 20, 4, 161, True, "ambiguous", tree=plain.tree)
        finally:
            assert L.pllhip_set_sharding(0, None)
        with shard:
            assert L.pllhip_shard_count(shard.p) == 2 and L.pllhip_shard_count(plain.p) == 1
            triples = triples_of(plain.tree)
            refs = references(plain, triples)
            a = check_batch(plain, triples, tally, "plain", refs)
            b = check_batch(shard, triples, tally, "two shards", refs)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
    tally.close("S=20 R=4 two shards")


@pytest.mark.gpu
@pytest.mark.parametrize("states,rate_cats", [(20, 4), (32, 4), (16, 4), (4, 4), (61, 4)])
def test_block_loop_with_a_capped_grid(product, monkeypatch, states, rate_cats):
    """PLLHIP_ANC_BLOCKS = 1 and 2 at 130 and 1031 sites: the 33 blocks of 1031 sites go over 4 or 8 waves, up to
    nine blocks a wave and unevenly, so the wave-private tile is reused; the grid-stride loops of the other kernels go
    round up to five times.  Everything bit-identical to the uncapped run, which is within the bound."""
    tally = Tally()
    for nsites in (130, 1031):
        monkeypatch.delenv("PLLHIP_ANC_BLOCKS", raising=False)
        with build_case(product, states, rate_cats, nsites, True, "ambiguous") as inst:
            triples = triples_of(inst.tree)
            free = check_batch(inst, triples, tally, f"N={nsites}")
            for cap in ("1", "2"):
                monkeypatch.setenv("PLLHIP_ANC_BLOCKS", cap)
                capped = run_batch(inst, triples)
                for x, y in zip(free, capped):
                    assert np.array_equal(x, y), (nsites, cap)
            monkeypatch.setenv("PLLHIP_ANC_BLOCKS", "0")
            for x, y in zip(free, run_batch(inst, triples)):
                assert np.array_equal(x, y)
    tally.close(f"S={states} R={rate_cats} capped grid")


@pytest.mark.gpu
@pytest.mark.parametrize("inputs", ["mixture", "ambiguous"])
@pytest.mark.parametrize("states,rate_cats", [(4, 4), (20, 4), (61, 4), (10, 4)])
def test_per_call_form_against_the_reference(product, states, rate_cats, inputs):
    """pll_compute_node_ancestral on the product (k_node_ancestral): a serial sum per thread, the same bound"""
    tally = Tally()
    for coded in (True, False):
        with build_case(product, states, rate_cats, 130, coded, inputs) as inst:
            for k, triple in enumerate(triples_of(inst.tree)):
                tally.check(inst, ar.reference(inst, *triple), per_call(inst, triple), where=f"coded={coded} entry {k}")
    tally.close(f"S={states} R={rate_cats} per-call form {inputs}")
