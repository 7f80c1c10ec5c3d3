"""Site categories on the CPU: tests/sitecat_reference.py (numpy.longdouble, bounds derived there) against a brute-force
enumeration, and the evaluation driver's host path (pllhip_eval_site_rates, pllhip_eval_optimize_rate_weights on the
oracle: plain C from the partition's host arrays) against the reference.  The device path is checked against the same
reference in tests/test_sitecat_gpu.py, so the host path is the independent second implementation.

`category` is checked exactly against the call's own table and against the reference on every row whose two largest
reference posteriors are further apart than both bounds; the reference alone may exclude at most 1 % of the rows that
are not all zero."""
import itertools

import numpy as np
import pytest

import pllhip_ctypes as pc
import sitecat_reference as sr
from test_ancestral_exact import ambiguity_map, towards

LD = np.longdouble
FULL = pc.PLLHIP_SITECAT_POSTERIORS


def cherry_of(tree):
    """(tip, tip, matrix, matrix) of the first operation whose children are both tips"""
    return next((op[2], op[5], op[3], op[6]) for op in tree.ops if op[2] < tree.ntips and op[5] < tree.ntips)


def driver_case(lib, states, rate_cats, nsites, ntips=9, inputs="plain", pinv=None, attributes=0, zero_cherry=False,
                alpha=None, constant=0, weights=None, brlen_scale=1.0):
    """an Evaluation with one partition.  inputs: 'plain', 'mixture' (params_indices 0, 1, 0, 1, unequal category
    weights) or 'ambiguous' (gaps and two partial codes at every tip, the mixture as well); pinv: a proportion, or one
    per rate matrix of a mixture; zero_cherry: both pendant edges of a cherry have length 0, so the sites at which its
    tips disagree have likelihood 0; constant: that many leading sites hold one state at every tip; brlen_scale: a factor
    on every branch length (long branches on a deep tree: even constant sites get scaled)"""
    tree = pc.Tree(ntips, 42, 43)
    tree.brlens = tree.brlens * brlen_scale
    codes = pc.random_codes(ntips, nsites, states, 44)
    if zero_cherry:
        ta, tb, ma, mb = cherry_of(tree)
        tree.brlens[ma] = tree.brlens[mb] = 0.0
        codes[tb, ::3] = codes[ta, ::3]
    for n in range(constant):
        codes[:, n] = n % states
    ev = pc.Evaluation(lib, tree.newick(), nparts=1)
    placed = np.zeros_like(codes)
    for k in range(ntips):                       # the sequence of tip k sits on the leaf labelled t<k>
        placed[ev.tip_clv[k]] = codes[k]
    mixed = inputs != "plain" and rate_cats > 1
    kw = {}
    if pinv is not None:
        kw = {"mixture_pinv": list(pinv)} if mixed else {"mixture_pinv": [pinv]}
    inst = pc.build_instance(lib, states=states, rate_cats=rate_cats, ntips=ntips, nsites=nsites, coded=True, alpha=alpha,
                             tree=tree, codes=placed, attributes=attributes,
                             mixture=[r % 2 for r in range(rate_cats)] if mixed else None, **kw)
    if mixed or weights is not None:
        w = pc._f64(np.arange(1.0, rate_cats + 1.0) / (rate_cats * (rate_cats + 1) / 2) if weights is None else weights)
        inst.L.pll_set_category_weights(inst.p, w.ctypes.data_as(pc.c_double_p))
    if inputs == "ambiguous":
        cmap, (c1, c2) = ambiguity_map(states)
        rnd = pc.splitmix64(49, ntips * nsites).reshape(ntips, nsites)
        for t in range(ntips):
            seq = (placed[t] + 48).astype(np.uint8)
            seq[rnd[t] % np.uint64(5) == 0] = ord("-")
            seq[rnd[t] % np.uint64(7) == 1] = ord(c1)
            seq[rnd[t] % np.uint64(11) == 2] = ord(c2)
            seq[:constant] = (placed[t][:constant] + 48).astype(np.uint8)
            inst.set_tip_states(t, cmap, seq.tobytes())
    if not ev.L.pllhip_eval_set_partition(ev.ev, 0, inst.p, inst.params_p):
        raise RuntimeError(lib.errmsg)
    ev.parts.append(inst)
    return ev, inst


class Tally:
    def __init__(self):
        self.rows = self.excluded = self.zero = 0
        self.worst = {}

    def within(self, name, got, ref, k, where, floor=None):
        frac = sr.worst(got, ref, k, floor)
        self.worst[name] = max(self.worst.get(name, 0.0), frac)
        assert frac <= 1.0, f"{where}: {name} is {frac:.3g} of its bound"

    def check(self, inst, tab, got, where, weights=None, m=None, rho=None, with_rates=True):
        """got: a pc.SitePosteriors with the full table; tab: the reference table"""
        S, R, N = inst.S, inst.R, len(tab.c)
        ref = sr.posteriors(tab.A, tab.B, tab.c, weights, rho, m)
        floor = sr.floor_of(ref.T)
        self.within("posterior", got.posterior, ref.post, sr.k_post(S, R), where, floor[:, None])
        if with_rates:
            self.within("rate", got.rate, ref.rate, sr.k_rate(S, R), where, sr.floor_of(ref.T, R * np.max(rho)))
            self.within("invariant_prob", got.invariant_prob, ref.inv, sr.k_inv(S, R), where, floor)
            # ... and everything adds up to 1 (to the roundings of the R + 1 terms and their sum)
            total = got.posterior.sum(axis=1) + got.invariant_prob
            live = ref.T > 0
            assert np.all(np.abs(total[live].astype(LD) - 1) <= float(2 * (sr.k_post(S, R) + R + 1)) * sr.U), where
        self.within("expected", got.expected, ref.expected, sr.k_exp(S, R, N), where, (ref.m.astype(LD) * floor).sum())
        fin = np.isfinite(ref.lnl)
        assert np.array_equal(np.isneginf(got.lnl), ~fin), where
        frac = float(np.max(np.abs(got.lnl[fin].astype(LD) - ref.lnl[fin]) / sr.lnl_bound(ref, S, R)[fin])) if fin.any() else 0.0
        self.worst["lnl"] = max(self.worst.get("lnl", 0.0), frac)
        assert frac <= 1.0, f"{where}: lnl is {frac:.3g} of its bound"
        if np.isfinite(ref.loglh):
            assert abs(LD(got.loglh) - ref.loglh) <= sr.loglh_bound(ref, S, R), where
        else:
            assert got.loglh == -np.inf, where
        # the summary: exactly against the call's own table ...
        assert np.array_equal(got.category, np.argmax(got.posterior, axis=1).astype(np.uint8)), where
        assert np.array_equal(got.category_prob, got.posterior.max(axis=1)), where
        # ... and against the reference wherever it decides
        clear, zero = sr.clear_rows(ref.post, S, R)
        assert np.array_equal(got.category[clear], ref.category[clear]), where
        assert not got.posterior[zero].any() and not got.category[zero].any() and not got.category_prob[zero].any(), where
        if with_rates:
            assert not got.rate[zero].any(), where
        self.rows += int((~zero).sum())
        self.zero += int(zero.sum())
        self.excluded += int((~clear & ~zero).sum())
        return ref

    def close(self, label):
        print(f"sitecat {label}: worst fractions of the bounds {{{', '.join(f'{k} {v:.3f}' for k, v in self.worst.items())}}}; "
              f"{self.rows} rows, {self.excluded} excluded, {self.zero} all zero")
        assert self.excluded * 100 <= self.rows, (self.excluded, self.rows)


# ---------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------
def test_reference_against_brute_force(oracle):
    """5 tips, 4 states, 2 categories, 3 sites with a partial code and a gap: l[n][r] at the root edge is the joint
    probability of the data and category r summed over all 4^3 assignments of the three inner nodes, written out edge by
    edge in longdouble; p-inv 0, no scaling"""
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
        pi = np.asarray(pc.DNA_FREQS, dtype=LD)
        inner = list(range(ntips, 2 * ntips - 2))
        want = np.zeros((3, R), dtype=LD)
        for site in range(3):
            mask = [int(cmap[ord(s[site])]) for s in seqs]
            for r in range(R):
                for assign in itertools.product(range(S), repeat=3):
                    x = dict(zip(inner, assign))
                    joint = pi[x[t.root_a]]
                    for m, (u, v) in enumerate(t.edges):
                        if u < ntips or v < ntips:
                            tip, nd = (u, v) if u < ntips else (v, u)
                            joint = joint * sum(P[m][r, x[nd], j] for j in range(S) if (mask[tip] >> j) & 1)
                        else:
                            a, b = (u, v) if towards(t, t.root_a, u) < towards(t, t.root_a, v) else (v, u)
                            joint = joint * P[m][r, x[a], x[b]]
                    want[site, r] += joint
        tab = sr.reference(inst, t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix)
        assert tab.A.dtype == LD and tab.A.shape == (3, R) and not tab.B.any() and not tab.c.any()
        # (the reference starts from the oracle's fp64 vectors below root_a: two levels of some 8 roundings each)
        assert np.all(np.abs(tab.A - want) <= 64 * sr.U * want)
        # posteriors per category and the site likelihood from the enumeration
        w = np.full(R, LD(1) / R)
        po = sr.posteriors(tab.A, tab.B, tab.c, w)
        T = (w[None, :] * want).sum(axis=1)
        assert np.all(np.abs(po.post - w[None, :] * want / T[:, None]) <= 200 * sr.U)
        _, persite = inst.edge_lnl(t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix, persite=True)
        assert np.all(np.abs(persite.astype(LD) - np.log(T)) <= 200 * sr.U * np.abs(np.log(T)))


# (states, rate_cats, keyword arguments of driver_case): p-inv on and off, a mixture with unequal weights, per-rate
# scalers on a deep tree (with and without invariant terms, i.e. with the descaled sites), ambiguity codes, all-zero rows
CASES = {
    "dna": (4, 4, {}),
    "dna-pinv": (4, 4, {"pinv": 0.25, "constant": 6}),
    "protein": (20, 4, {}),
    "protein-pinv": (20, 4, {"pinv": 0.2, "constant": 6}),
    "dna-mixture": (4, 4, {"inputs": "mixture"}),
    "protein-mixture-pinv": (20, 4, {"inputs": "mixture", "pinv": (0.3, 0.0), "constant": 6}),
    "dna-ambiguous": (4, 4, {"inputs": "ambiguous", "pinv": (0.1, 0.2), "constant": 4}),
    "protein-ambiguous": (20, 4, {"inputs": "ambiguous"}),
    "dna-deep": (4, 4, {"ntips": 300, "alpha": 2.0, "brlen_scale": 40.0, "pinv": 0.2, "constant": 6}),
    "dna-rate-scalers": (4, 4, {"ntips": 300, "alpha": 0.3, "attributes": pc.PLL_ATTRIB_RATE_SCALERS}),
    "dna-rate-scalers-pinv": (4, 4, {"ntips": 300, "alpha": 2.0, "brlen_scale": 40.0,
                                     "attributes": pc.PLL_ATTRIB_RATE_SCALERS, "pinv": 0.2, "constant": 6}),
    "protein-rate-scalers": (20, 4, {"ntips": 150, "alpha": 0.3, "attributes": pc.PLL_ATTRIB_RATE_SCALERS}),
    "dna-zero": (4, 4, {"zero_cherry": True}),
    "protein-zero": (20, 4, {"zero_cherry": True, "inputs": "mixture"}),
}


def edge_reference(ev, inst):
    pc_, psc, cc, csc, m = ev.root_edge()
    return sr.reference(inst, pc_, psc, cc, csc, m)


@pytest.mark.parametrize("name", list(CASES))
def test_site_rates_of_the_driver_against_the_reference(oracle, name):
    states, rate_cats, kw = CASES[name]
    tally = Tally()
    for nsites in (33, 130):
        ev, inst = driver_case(oracle, states, rate_cats, nsites, **kw)
        with ev:
            total = ev.loglh()
            got, = ev.site_rates(FULL)
            plain, = ev.site_rates(0)
            assert plain.posterior is None
            for f in ("rate", "category", "category_prob", "invariant_prob", "lnl", "expected"):
                assert np.array_equal(getattr(plain, f), getattr(got, f)), f
            tab = edge_reference(ev, inst)
            _, q, w, rho, m, inv = sr.model_of(inst)
            ref = tally.check(inst, tab, got, f"{name} N={nsites}", w, m, rho)
            # log T - c 256 ln 2 is the oracle's per-site log-likelihood, and their sum its total
            _, persite = ev.persite_lnl(0)
            fin = np.isfinite(ref.lnl)
            assert np.array_equal(np.isneginf(persite), ~fin)
            assert np.all(np.abs(persite[fin].astype(LD) - ref.lnl[fin]) <= sr.lnl_bound(ref, states, rate_cats)[fin])
            if np.isfinite(ref.loglh):
                assert abs(LD(total) - ref.loglh) <= sr.loglh_bound(ref, states, rate_cats)
            # the case holds what its name says
            if "pinv" in kw:
                assert (inv[:kw["constant"]] >= 0).all() and tab.B.any() and (got.invariant_prob > 0).any()
            else:
                assert not got.invariant_prob.any()
            if kw.get("ntips", 0) >= 150:
                counts = sr.counts_of(inst, ev.root_edge()[1]) + sr.counts_of(inst, ev.root_edge()[3])
                assert counts.any()
                if kw.get("attributes") and kw["alpha"] < 1:
                    assert (counts.min(axis=1) != counts.max(axis=1)).any()
                if "pinv" in kw:
                    assert not tab.c[:kw["constant"]].any() and counts[:kw["constant"]].all()    # the descaled sites
            if kw.get("zero_cherry"):
                assert (~fin).any() and fin.any()
    tally.close(name)
    assert bool(tally.zero) == bool(kw.get("zero_cherry"))


def test_unknown_flags_and_a_remote_partition_are_refused(oracle):
    ev, inst = driver_case(oracle, 4, 4, 33)
    with ev:
        with pytest.raises(RuntimeError):
            ev.site_rates(2)
        with pytest.raises(RuntimeError):
            ev.optimize_rate_weights(partition=1)


EM_CASES = ["dna", "protein", "dna-pinv", "protein-mixture-pinv", "dna-rate-scalers-pinv"]


@pytest.mark.parametrize("name", EM_CASES)
def test_rate_weights_of_the_driver_step_by_step(oracle, name):
    states, rate_cats, kw = CASES[name]
    nsites = 130
    start = np.array([0.55, 0.25, 0.15, 0.05])
    ev, inst = driver_case(oracle, states, rate_cats, nsites, weights=start, **kw)
    with ev:
        before = ev.loglh()
        tab = edge_reference(ev, inst)
        _, q, w0, rho, m, inv = sr.model_of(inst)
        after, fit = ev.optimize_rate_weights(0, epsilon=1e-4, max_iterations=12)
        n = len(fit.trail_loglh)
        assert 3 <= n <= 13 and fit.iterations == n - 1
        assert np.array_equal(fit.trail_weights[0], w0) and np.array_equal(fit.trail_weights[-1], fit.weights)
        kL = []
        for i in range(n):
            step, L = sr.em_step(tab.A, tab.B, tab.c, fit.trail_weights[i], m)
            po = sr.posteriors(tab.A, tab.B, tab.c, fit.trail_weights[i], None, m)
            kL.append(sr.loglh_bound(po, states, rate_cats))
            assert abs(LD(fit.trail_loglh[i]) - L) <= kL[i], i
            if i + 1 < n:           # every step is the reference's step from the trail's own iterate
                assert sr.worst(fit.trail_weights[i + 1], step, sr.k_step(states, rate_cats, nsites)) <= 1.0, i
        for i in range(1, n):       # EM never loses likelihood
            assert LD(fit.trail_loglh[i]) >= LD(fit.trail_loglh[i - 1]) - (kL[i] + kL[i - 1]), i
        assert fit.trail_loglh[-1] > fit.trail_loglh[0] + 1e-3
        if fit.iterations < 12:
            assert fit.trail_loglh[-1] - fit.trail_loglh[-2] < 1e-4
        assert abs(LD(fit.weights.sum()) - 1) <= (rate_cats + 2) * sr.U
        # installed: a full re-evaluation with the new weights returns the reported value
        assert np.array_equal(sr.model_of(inst)[2], fit.weights)
        full = ev.loglh()
        assert after == full and abs(LD(full) - LD(fit.trail_loglh[-1])) <= 2 * kL[-1]
        assert full > before


def test_rate_weights_refuse_an_ascertainment_partition(oracle):
    ev, inst = driver_case(oracle, 4, 4, 33, attributes=pc.PLL_ATTRIB_AB_FLAG | pc.PLL_ATTRIB_AB_LEWIS)
    with ev:
        inst.set_asc(pc.PLL_ATTRIB_AB_LEWIS)
        ev.loglh()
        assert len(ev.site_rates(0)[0].lnl) == 33            # the table and the posteriors ignore the correction
        with pytest.raises(RuntimeError, match="ascertainment"):
            ev.optimize_rate_weights(0)


def test_rate_weights_name_a_site_without_likelihood(oracle):
    ev, inst = driver_case(oracle, 4, 4, 33, zero_cherry=True)
    with ev:
        ev.loglh()
        bad = int(np.flatnonzero(np.isneginf(ev.site_rates(0)[0].lnl))[0])
        with pytest.raises(RuntimeError, match=f"site {bad} "):
            ev.optimize_rate_weights(0)
