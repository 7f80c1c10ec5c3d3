"""Sampled ancestral states on the CPU: the evaluation driver's host path (pllhip_eval_sample_ancestral on the oracle:
the contract in plain C from the partition's host arrays) byte for byte against tests/ancsample_reference.py, the
formula against a brute-force posterior, sampled frequencies against the marginals, tips, dropped sites, ranges and
refusals.  The device path is held to the same reference in tests/test_ancsample_gpu.py, so the host path is the
independent second implementation.  The refusals of the edge-list form need a partition on a device and are tested
there; so is the order of a caller's edge list (the driver builds its own)."""
import itertools

import numpy as np
import pytest

import ancestral_reference as ar
import ancsample_reference as asr
import pllhip_ctypes as pc
from test_sitecat_cpu import driver_case

LD = np.longdouble
TIPS, COMPONENT = pc.PLLHIP_ANCS_TIPS, pc.PLLHIP_ANCS_COMPONENT

# (states, rate_cats, keyword arguments of test_sitecat_cpu.driver_case, flags)
SHAPES = {
    "dna-gamma-pinv": (4, 4, {"pinv": 0.25, "constant": 6}, 0),
    "binary-one-category": (2, 1, {"ntips": 5}, 0),
    "five-states": (5, 3, {"ntips": 7}, 0),
    "protein-mixture-pinv": (20, 4, {"inputs": "mixture", "pinv": (0.3, 0.1), "constant": 6}, 0),
    "dna-ambiguous-tips": (4, 4, {"inputs": "ambiguous", "pinv": (0.1, 0.2), "constant": 4}, TIPS),
    "protein-ambiguous-tips": (20, 4, {"inputs": "ambiguous"}, TIPS),
}


def reference_of(ev, inst, seed, replicates, first=0, flags=0, alphabet=None):
    edges, root_edge = asr.driver_edges(ev)
    x = asr.gather(inst, edges, root_edge, asr.host_table)
    return x, asr.sample(x, seed, replicates, first, tips=bool(flags & TIPS), alphabet=alphabet)


@pytest.mark.parametrize("name", list(SHAPES))
def test_driver_bytes_equal_the_reference(oracle, name):
    states, rate_cats, kw, flags = SHAPES[name]
    ev, inst = driver_case(oracle, states, rate_cats, 67, **kw)
    with ev:
        ev.loglh()
        got, = ev.sample_ancestral(20261021, replicates=3, flags=flags)
        x, (out, comp, dropped) = reference_of(ev, inst, 20261021, 3, flags=flags)
        assert got.out.shape == out.shape and np.array_equal(got.clv_index, np.arange(out.shape[1]))
        assert np.array_equal(got.out, out)
        assert np.array_equal(got.component, comp)
        assert got.dropped == dropped == 0
        # the case holds what its name says
        inner = got.out[:, inst.tips:2 * inst.tips - 2]
        assert (inner < states).all() and len(np.unique(inner)) == states
        assert (got.out[:, 2 * inst.tips - 2:] == 255).all()
        assert ((got.out[:, :inst.tips] == 255).all()) == (not flags & TIPS)
        if "pinv" in kw:
            drawn = (got.component & 0x80) != 0
            assert drawn.any() and (x.invariant[np.nonzero(drawn)[1]] >= 0).all()
            rows = got.out[:, inst.tips:2 * inst.tips - 2]
            assert (rows.transpose(0, 2, 1)[drawn] == x.invariant[np.nonzero(drawn)[1]][:, None]).all()
        else:
            assert not (got.component & 0x80).any()
        if rate_cats > 1:
            assert len(np.unique(got.component & 0x7f)) > 1


def test_the_formula_against_a_brute_force_posterior(oracle):
    """4 tips, 2 states, 2 categories with unequal weights and p-inv: for every joint assignment of (component, the two
    inner states) the product of the reference's three conditional probabilities is the posterior written out edge by
    edge in longdouble from the oracle's own matrices, within asr.formula_bound.  No sampling."""
    S, R, ntips, nsites, q = 2, 2, 4, 16, 0.2
    codes = np.array([[(n >> t) & 1 for n in range(nsites)] for t in range(ntips)], dtype=np.uint8)    # every pattern
    t = pc.Tree(ntips, 7, 8)
    t.set_root_edge(next(k for k, (u, v) in enumerate(t.edges) if u >= ntips and v >= ntips))
    inst = pc.build_instance(oracle, S, R, ntips, nsites, tree=t, codes=codes, pinv=q)
    w = np.array([0.3, 0.7])
    inst.L.pll_set_category_weights(inst.p, pc._f64(w).ctypes.data_as(pc.c_double_p))
    with inst:
        pc.full_traversal(inst)
        root_edge = (t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b))
        assert t.root_a >= ntips and t.root_b >= ntips
        x = asr.gather(inst, pc.tree_edges(t, t.root_a), root_edge, asr.host_table)
        P = {m: np.asarray(inst.get_pmatrix(m), dtype=LD) for m in range(t.nedges)}
        pi = np.asarray(x.freqs[0], dtype=LD)
        below = {node: [(c, m) for (p, c, m) in x.edges if p == node and c < ntips] for node in (t.root_a, t.root_b)}
        mass = x.comp_mass()
        worst, bound = 0.0, asr.formula_bound(S, R)
        for n in range(nsites):
            # the exact joint weights of (component, root state, other state)
            exact = {}
            for r in range(R):
                for a, b in itertools.product(range(S), repeat=2):
                    v = LD(w[r]) * (1 - LD(q)) * pi[a] * P[x.m0][r, a, b]
                    for node, s in ((t.root_a, a), (t.root_b, b)):
                        for c, m in below[node]:
                            v = v * P[m][r, s, codes[c, n]]
                    exact[(2 * r, a, b)] = v
                inv = x.invariant[n]
                if inv >= 0:
                    exact[(2 * r + 1, inv, inv)] = LD(w[r]) * LD(q) * pi[inv]
            total = sum(exact.values())
            seen = LD(0)
            for k in range(2 * R):
                r = np.array([k >> 1])
                f1 = LD(mass[n, k]) / LD(asr.cumulate(mass[n])[-1])
                if k & 1:
                    if mass[n, k] > 0:
                        key = (k, x.invariant[n], x.invariant[n])
                        worst = max(worst, float(abs(f1 - exact[key] / total) / (exact[key] / total)))
                        seen += f1
                    else:
                        assert (k, x.invariant[n], x.invariant[n]) not in exact or x.invariant[n] < 0
                    continue
                om = x.root_mass(np.repeat(r, nsites))[n]
                for a, b in itertools.product(range(S), repeat=2):
                    oe = x.edge_mass(t.root_b, x.m0, np.repeat(r, nsites), np.full(nsites, a))[n]
                    got = f1 * (LD(om[a]) / LD(asr.cumulate(om)[-1])) * (LD(oe[b]) / LD(asr.cumulate(oe)[-1]))
                    want = exact[(k, a, b)] / total
                    worst = max(worst, float(abs(got - want) / want))
                    seen += got
            assert abs(seen - 1) <= 8 * bound
        print(f"formula: worst relative difference {worst:.3g}, bound {bound:.3g}")
        assert worst <= bound
        # a tip below either node: its conditional probability of the observed state is 1
        for node in (t.root_a, t.root_b):
            for c, m in below[node]:
                oe = x.edge_mass(c, m, np.zeros(nsites, dtype=np.int64), np.ones(nsites, dtype=np.int64))
                assert ((oe > 0).sum(axis=1) == 1).all() and (np.argmax(oe, axis=1) == codes[c]).all()


FREQ_SEED, FREQ_REPLICATES = 7, 2048


def test_sampled_frequencies_against_the_marginals(oracle):
    """9 tips, 4 states, 4 categories, 40 sites, 2048 replicates of one seed: the frequency of every state at every
    inner node lies within 5 sqrt(p (1 - p) / B) + 1 / B of the marginal posterior of pllhip_eval_compute_ancestral.
    The seed was fixed after the numpy reference was seen to pass with no entry outside; the driver's bytes are the
    reference's (checked here on the first replicates)."""
    B = FREQ_REPLICATES
    ev, inst = driver_case(oracle, 4, 4, 40)
    with ev:
        ev.loglh()
        anc = ev.compute_ancestral(pc.PLLHIP_ANC_PROBS)
        got, = ev.sample_ancestral(FREQ_SEED, replicates=B)
        _, (out, comp, _) = reference_of(ev, inst, FREQ_SEED, 16)
        assert np.array_equal(got.out[:16], out) and np.array_equal(got.component[:16], comp)
        outside = 0
        for i, clv in enumerate(anc.node_clv):
            p = anc.probs[i].reshape(40, 4)
            f = np.stack([(got.out[:, clv, :] == s).mean(axis=0) for s in range(4)], axis=1)
            outside += int((np.abs(f - p) > 5 * np.sqrt(p * (1 - p) / B) + 1.0 / B).sum())
        assert len(anc.node_clv) == 7 and outside == 0


@pytest.mark.parametrize("states", [4, 20])
def test_tip_rows_are_compatible_with_the_codes(oracle, states):
    ev, inst = driver_case(oracle, states, 4, 67, inputs="ambiguous")
    with ev:
        ev.loglh()
        got, = ev.sample_ancestral(11, replicates=4, flags=TIPS)
        ambiguous = 0
        for tip in range(inst.tips):
            mask = ar.clv_of(inst, tip)[:, 0, :] > 0                   # [site][state]
            rows = got.out[:, tip, :]
            assert (rows < states).all()
            assert mask[np.arange(67)[None, :], rows].all()
            single = mask.sum(axis=1) == 1
            assert (rows[:, single] == np.argmax(mask, axis=1)[single][None, :]).all()
            ambiguous += int((~single).sum())
        assert ambiguous > 20


@pytest.mark.parametrize("states,inputs", [(4, "plain"), (20, "mixture")])
def test_dropped_sites(oracle, states, inputs):
    """the zero_cherry construction of test_sitecat_cpu.py: the sites with likelihood 0 are 0xFF in every row, every
    replicate and the component, and are counted once"""
    ev, inst = driver_case(oracle, states, 4, 67, zero_cherry=True, inputs=inputs)
    with ev:
        ev.loglh()
        _, persite = ev.persite_lnl(0)
        dead = np.isneginf(persite)
        assert dead.any() and not dead.all()
        got, = ev.sample_ancestral(5, replicates=3, flags=TIPS)
        assert got.dropped == int(dead.sum())
        assert (got.out[:, :, dead] == 255).all() and (got.component[:, dead] == 255).all()
        assert (got.out[:, :2 * inst.tips - 2][:, :, ~dead] < states).all() and (got.component[:, ~dead] != 255).all()
        _, (out, comp, dropped) = reference_of(ev, inst, 5, 3, flags=TIPS)
        assert np.array_equal(got.out, out) and np.array_equal(got.component, comp) and dropped == got.dropped


def test_replicate_ranges_and_the_alphabet(oracle):
    ev, inst = driver_case(oracle, 4, 4, 67, pinv=0.25, constant=6)
    with ev:
        ev.loglh()
        whole, = ev.sample_ancestral(3, replicates=5)
        part, = ev.sample_ancestral(3, replicates=3, first_replicate=2)
        assert np.array_equal(part.out, whole.out[2:5]) and np.array_equal(part.component, whole.component[2:5])
        other, = ev.sample_ancestral(4, replicates=5)
        assert not np.array_equal(other.out, whole.out)
        text, = ev.sample_ancestral(3, replicates=5, alphabet="ACGT")
        want = np.where(whole.out == 255, 255, np.frombuffer(b"ACGT", np.uint8)[np.minimum(whole.out, 3)])
        assert np.array_equal(text.out, want) and np.array_equal(text.component, whole.component)
        # the reference does not depend on the order of its edge list either
        edges, root_edge = asr.driver_edges(ev)
        order = np.argsort(pc.splitmix64(9, len(edges[0])))
        x = asr.gather(inst, tuple(a[order] for a in edges), root_edge, asr.host_table)
        out, comp, _ = asr.sample(x, 3, 2)
        assert np.array_equal(out, whole.out[:2]) and np.array_equal(comp, whole.component[:2])


def test_the_driver_is_left_as_it_was(oracle):
    ev, inst = driver_case(oracle, 4, 4, 67)
    with ev:
        before = ev.loglh()
        root = ev.root_edge()
        lengths = [rec.contents.length for rec in ev.records()]
        ev.set_transient(1)
        ev.sample_ancestral(3, replicates=2)
        assert ev.root_edge() == root and [rec.contents.length for rec in ev.records()] == lengths
        assert ev.loglh(incremental=True) == before and ev.loglh() == before


def test_refusals_write_nothing(oracle):
    ev, inst = driver_case(oracle, 4, 4, 33)
    with ev:
        ev.loglh()
        for kw, what in (({"replicates": 0}, "zero replicates"), ({"flags": 4}, "unknown flags"),
                         ({"alphabet": "ACG"}, "alphabet"), ({"replicates": 2, "first_replicate": 2 ** 32 - 1}, "2\\^32")):
            args = {"replicates": 1, **kw}
            oracle.errno = 0
            with pytest.raises(RuntimeError, match=what):
                ev.sample_ancestral(1, **args)
        oracle.errno = 0
        assert not ev.L.pllhip_eval_sample_ancestral(ev.ev, None) and oracle.errno != 0
        w = inst.p.contents.rate_weights
        saved = w[1]
        for bad, what in ((-0.25, "weight 1"), (float("nan"), "weight 1")):
            w[1] = bad
            with pytest.raises(RuntimeError, match=what):
                ev.sample_ancestral(1)
        w[1] = saved
        for r in range(4):
            w[r] = 0.0
        with pytest.raises(RuntimeError, match="add up to 0"):
            ev.sample_ancestral(1)
        for r in range(4):
            w[r] = 0.25
        assert ev.sample_ancestral(1)[0].out.shape[2] == 33


def test_symbols_are_declared():
    for n in ("pllhip_sample_ancestral_edges", "pllhip_sample_ancestral_utree", "pllhip_ancsample_last_times"):
        assert n in pc.PLLHIP_H_FUNCTIONS
    for n in ("pllhip_eval_sample_ancestral", "pllhip_eval_destroy_sampled_ancestral"):
        assert n in pc.PLLHIP_EVAL_H_FUNCTIONS
