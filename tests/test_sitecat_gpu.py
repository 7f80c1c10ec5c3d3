"""The site-category kernels (kernels_sitecat.hpp, kernels_sitecat_sums.hpp; pllhip_sitecat_*) against
tests/sitecat_reference.py: table, posteriors, site rates, invariant parts, lnl and expected counts in numpy.longdouble
from what the engine itself holds, under the bounds derived there.  lnl is also held against the per-site values of
pll_compute_edge_loglikelihood on the same edge; the summary exactly against the call's own table and against the
reference wherever it decides (tests/test_sitecat_cpu.py, Tally)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pllhip_ctypes as pc
import sitecat_reference as sr
from test_ancestral_exact import build_case, triples_of
from test_sitecat_cpu import FULL, Tally, driver_case

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
SITES = [1, 2, 31, 32, 33, 64, 130]

# (states, rate_cats): the family whose table kernel has to run it (sitecat_edge_table dispatches on it)
KERNELS = {
    (4, 4): b"s4-valu", (4, 1): b"s4-valu",
    (4, 3): b"s16-mfma", (5, 4): b"s16-mfma",
    (20, 12): b"s16-mfma",                     # five k-steps and the 4 x 4 x 4 tail under twelve rates of fragments
    (20, 4): b"s20-mfma", (20, 1): b"s20-mfma",
    (61, 4): b"s61-mfma",                      # k_sitecat_generic on blocked rows
    (20, 16): b"generic",                      # k_sitecat_generic on the API layout
}
SHAPES = list(KERNELS)


def edge_of(inst, triple):
    node, other, m = triple
    t = inst.tree
    return node, t.scaler_of(node), other, t.scaler_of(other), m


def unequal_weights(inst):
    """category weights 1 : 2 : ... : R.  Under equal weights the triples with the zero-length and the saturated matrix
    tie exactly (every category has the same table entry there) and the reference could name no category."""
    w = pc._f64(np.arange(1.0, inst.R + 1.0) / (inst.R * (inst.R + 1) / 2))
    inst.L.pll_set_category_weights(inst.p, w.ctypes.data_as(pc.c_double_p))


def check_edge(inst, triple, tally, where, weights=None):
    """one set: table, posteriors (twice: the sums repeat bit for bit), lnl against the edge log-likelihood"""
    S, R = inst.S, inst.R
    edge = edge_of(inst, triple)
    tab = sr.reference(inst, *edge)
    _, q, w, rho, m, inv = sr.model_of(inst)
    with pc.SiteCat.edge(inst, *edge) as sc:
        assert (sc.sites, sc.cats) == (inst.N, R)
        A, B, c = sc.table()
        got = sc.posteriors(weights, FULL)
        again = sc.posteriors(weights, 0)
    tally.within("table", A, tab.A, sr.k_tab(S), where)
    tally.within("invariant table", B, tab.B, sr.k_tab(S), where)
    assert np.array_equal(c, tab.c), where
    ref = tally.check(inst, tab, got, where, w if weights is None else weights, m, rho)
    assert again.posterior is None and np.array_equal(again.loglh, got.loglh, equal_nan=True), where
    for f in ("rate", "category", "category_prob", "invariant_prob", "lnl", "expected"):
        assert np.array_equal(getattr(again, f), getattr(got, f)), (where, f)
    if weights is None:
        _, persite = inst.edge_lnl(*edge, persite=True)
        fin = np.isfinite(ref.lnl)
        assert np.array_equal(np.isneginf(persite), ~fin), where
        assert np.all(np.abs(persite[fin].astype(LD) - ref.lnl[fin]) <= sr.lnl_bound(ref, S, R)[fin]), where
    return A, B, c, got


@pytest.mark.gpu
@pytest.mark.parametrize("coded", [True, False], ids=["coded", "tip-vectors"])
@pytest.mark.parametrize("states,rate_cats", SHAPES)
def test_every_kernel_at_every_site_count(product, states, rate_cats, coded):
    """all four operand kinds (inner x inner, inner x tip, tip x inner, tip x tip, adjacent and not), among them the
    zero-length matrix between two tips: all-zero rows where they disagree"""
    tally = Tally()
    for nsites in SITES:
        with build_case(product, states, rate_cats, nsites, coded) as inst:
            assert product.lib.pllhip_partials_kernel_name(inst.p) == KERNELS[states, rate_cats]
            unequal_weights(inst)
            for k, triple in enumerate(triples_of(inst.tree)):
                check_edge(inst, triple, tally, f"N={nsites} entry {k} {triple}")
    tally.close(f"S={states} R={rate_cats} coded={coded}")
    assert tally.zero > 0


VARIANTS = [(S, R, v) for S, R in SHAPES for v in ("pinv", "mixture", "ambiguous-pinv") if R > 1 or v == "pinv"]


@pytest.mark.gpu
@pytest.mark.parametrize("states,rate_cats,variant", VARIANTS)
def test_pinv_mixture_and_ambiguity_codes(product, states, rate_cats, variant):
    tally = Tally()
    kw = {"pinv": {"mixture_pinv": [0.25]}, "mixture": {}, "ambiguous-pinv": {"mixture_pinv": [0.3, 0.0]}}[variant]
    inputs = {"pinv": "plain", "mixture": "mixture", "ambiguous-pinv": "ambiguous"}[variant]
    for nsites in (33, 130):
        for coded in (True, False):
            with build_case(product, states, rate_cats, nsites, coded, inputs, **kw) as inst:
                if variant != "mixture":
                    assert inst.p.contents.invariant
                unequal_weights(inst)
                for k, triple in enumerate(triples_of(inst.tree)):
                    check_edge(inst, triple, tally, f"{variant} N={nsites} coded={coded} entry {k}")
                # other weights than the set's own
                w = np.arange(rate_cats, 0.0, -1.0)
                check_edge(inst, triples_of(inst.tree)[0], tally, f"{variant} weights", weights=w / w.sum())
    tally.close(f"S={states} R={rate_cats} {variant}")


DEEP = [(4, 400, 4, 0), (20, 200, 4, 0), (61, 100, 4, 0), (4, 400, 4, pc.PLL_ATTRIB_RATE_SCALERS),
        (20, 200, 4, pc.PLL_ATTRIB_RATE_SCALERS), (61, 100, 4, pc.PLL_ATTRIB_RATE_SCALERS),
        (7, 250, 3, pc.PLL_ATTRIB_RATE_SCALERS), (20, 200, 3, pc.PLL_ATTRIB_RATE_SCALERS)]


@pytest.mark.gpu
@pytest.mark.parametrize("pinv", [0.0, 0.2])
@pytest.mark.parametrize("states,ntips,rate_cats,attributes", DEEP)
def test_scaled_vectors(product, states, ntips, rate_cats, attributes, pinv):
    """deep trees whose vectors carry scaler counts, per site and per (site, rate); with p-inv the sites that have an
    invariant term are brought to scale and their count is 0"""
    tally = Tally()
    tree = pc.Tree(ntips, 42, 43)
    kw = {"mixture_pinv": [pinv]} if pinv else {}
    codes = pc.random_codes(ntips, 65, states, 44)
    codes[:, :8] = (np.arange(8) % states)[None, :]
    with pc.build_instance(product, states=states, rate_cats=rate_cats, ntips=ntips, nsites=65, coded=True, tree=tree,
                           codes=codes, alpha=0.3 if states <= 20 else 1.0, attributes=attributes, **kw) as inst:
        pc.full_traversal(inst)
        unequal_weights(inst)
        top = tree.ops[-1]
        child, m = next((c, k) for c, k in ((top[2], top[3]), (top[5], top[6])) if c >= ntips)
        assert inst.get_scaler(tree.scaler_of(tree.root_a)).any()
        for k, triple in enumerate([(tree.root_a, child, m), (child, tree.root_a, m),
                                    (tree.root_a, tree.root_b, tree.root_matrix),
                                    (tree.root_b, tree.root_a, tree.root_matrix)]):
            A, B, c, got = check_edge(inst, triple, tally, f"{ntips} tips entry {k}")
            if pinv:
                assert B[:8].any() and not c[:8].any()
    tally.close(f"S={states} R={rate_cats} deep tree, attributes {attributes}, pinv {pinv}")


def driver_results(product, states, attributes=0, transient=False):
    ev, inst = driver_case(product, states, 4, 130, ntips=12, inputs="ambiguous", pinv=(0.2, 0.1), constant=4,
                           attributes=attributes)
    with ev:
        if transient:
            ev.set_transient(1)
        first = ev.loglh()
        got, = ev.site_rates(FULL)
        lnl, fit = ev.optimize_rate_weights(0, 1e-5, 8)
        assert ev.loglh() == lnl and lnl > first
        return got, fit, first, lnl


@pytest.mark.gpu
@pytest.mark.parametrize("states", [4, 20])
def test_driver_with_site_repeats_and_in_transient_mode(product, states):
    """through pllhip_eval_site_rates / pllhip_eval_optimize_rate_weights on the device: class nodes of site repeats and
    vectors that exist as their operation only are materialised by the reader; bit for bit the plain partition's results"""
    plain = driver_results(product, states)
    for other in (driver_results(product, states, attributes=pc.PLL_ATTRIB_SITE_REPEATS),
                  driver_results(product, states, transient=True)):
        for f in ("rate", "category", "category_prob", "invariant_prob", "lnl", "posterior", "expected"):
            assert np.array_equal(getattr(other[0], f), getattr(plain[0], f)), f
        assert np.array_equal(other[1].trail_weights, plain[1].trail_weights)
        assert np.array_equal(other[1].trail_loglh, plain[1].trail_loglh)
        assert other[2:] == plain[2:]


@pytest.mark.gpu
@pytest.mark.parametrize("states,rate_cats", [(4, 4), (20, 4), (5, 4)])
def test_unstored_vectors_are_stored_for_this_reader(product, states, rate_cats):
    """a traversal in transient mode leaves vectors out; a set that reads one gets it stored (need_clv), its results are
    those of the partition that stored everything, and what the partition computes afterwards is unchanged"""
    with build_case(product, states, rate_cats, 130, True, "ambiguous") as plain, \
            build_case(product, states, rate_cats, 130, True, "ambiguous") as lazy:
        lazy.set_transient(True)
        lnl = pc.full_traversal(lazy)
        lazy.set_transient(False)
        assert lnl == pc.full_traversal(plain)
        before = lazy.transient_stats().materialized
        for triple in triples_of(plain.tree):
            with pc.SiteCat.edge(plain, *edge_of(plain, triple)) as a, pc.SiteCat.edge(lazy, *edge_of(lazy, triple)) as b:
                for x, y in zip(a.table(), b.table()):
                    assert np.array_equal(x, y), triple
                assert np.array_equal(a.posteriors().lnl, b.posteriors().lnl)
        if not lazy.repeat_stats().cherries:        # (with class nodes the schedule, and what it leaves out, is another)
            assert lazy.transient_stats().skipped > 0 and lazy.transient_stats().materialized > before
        assert pc.full_traversal(lazy) == lnl


@pytest.mark.gpu
@pytest.mark.parametrize("states", [4, 20])
def test_driver_on_the_device_against_the_reference(product, states):
    tally = Tally()
    ev, inst = driver_case(product, states, 4, 130, ntips=12, inputs="mixture", pinv=(0.2, 0.0), constant=4,
                           weights=[0.55, 0.25, 0.15, 0.05])
    with ev:
        ev.loglh()
        got, = ev.site_rates(FULL)
        pc_, psc, cc, csc, m = ev.root_edge()
        tab = sr.reference(inst, pc_, psc, cc, csc, m)
        _, q, w, rho, pw, inv = sr.model_of(inst)
        tally.check(inst, tab, got, "driver", w, pw, rho)
        after, fit = ev.optimize_rate_weights(0, 1e-4, 12)
        check_trail(fit, tab, pw, states, 4, 130)
        assert abs(LD(fit.weights.sum()) - 1) <= 6 * sr.U
        assert np.array_equal(sr.model_of(inst)[2], fit.weights)
        assert abs(LD(ev.loglh()) - LD(fit.trail_loglh[-1])) <= 2 * sr.loglh_bound(sr.posteriors(tab.A, tab.B, tab.c, fit.weights, None, pw), states, 4)
    tally.close(f"driver S={states}")


def check_trail(fit, tab, m, S, R, N):
    """every step is the reference's step from the trail's own iterate; the log-likelihood never drops by more than
    the bounds of the two values"""
    n, kL = len(fit.trail_loglh), []
    for i in range(n):
        step, L = sr.em_step(tab.A, tab.B, tab.c, fit.trail_weights[i], m)
        kL.append(sr.loglh_bound(sr.posteriors(tab.A, tab.B, tab.c, fit.trail_weights[i], None, m), S, R))
        assert abs(LD(fit.trail_loglh[i]) - L) <= kL[i], i
        if i + 1 < n:
            assert sr.worst(fit.trail_weights[i + 1], step, sr.k_step(S, R, N)) <= 1.0, i
        if i:
            assert LD(fit.trail_loglh[i]) >= LD(fit.trail_loglh[i - 1]) - (kL[i] + kL[i - 1]), i
    assert np.array_equal(fit.trail_weights[-1], fit.weights) and fit.trail_loglh[-1] == fit.loglh
    assert fit.iterations == n - 1


@pytest.mark.gpu
def test_partition_is_left_as_it_was(product):
    """vectors, scaler counts and the counters other than reads are those of before, after every call"""
    with build_case(product, 20, 4, 130, True, "ambiguous", mixture_pinv=[0.2, 0.1]) as inst:
        t = inst.tree
        edge = (t.parent, t.scaler_of(t.parent), t.child, t.scaler_of(t.child), t.m_inner)
        state = lambda: (inst.get_clv(t.parent), inst.get_clv(t.child), inst.get_scaler(edge[1]), inst.get_scaler(edge[3]),
                         [getattr(inst.counters(), f) for f in ("partial_ops", "partial_launches", "site_updates",
                                                                "pmatrix_updates", "pmatrix_launches", "model_uploads")])
        before, lnl = state(), inst.edge_lnl(*edge)
        with pc.SiteCat.edge(inst, *edge) as sc:
            sc.table(), sc.posteriors(flags=FULL), sc.em_weights(1e-6, 4)
            for x, y in zip(before, state()):
                assert np.array_equal(x, y)
            assert inst.edge_lnl(*edge) == lnl
            # a set is a snapshot: it outlives changes of the partition
            po = sc.posteriors()
            w = pc._f64([0.7, 0.1, 0.1, 0.1])
            inst.L.pll_set_category_weights(inst.p, w.ctypes.data_as(pc.c_double_p))
            assert inst.edge_lnl(*edge) != lnl
            assert np.array_equal(sc.posteriors().lnl, po.lnl)


@pytest.mark.gpu
@pytest.mark.parametrize("states,rate_cats", [(4, 4), (5, 4), (20, 4), (61, 4), (20, 16)])
def test_capped_grid_in_a_child_process(product, tmp_path, states, rate_cats):
    """PLLHIP_SITECAT_BLOCKS=1 at 257 and 1000 sites: a wave walks up to eight site blocks, a thread four sites.
    Per-site outputs are bit-identical to the uncapped run; the sums repeat bit for bit at either cap."""
    import _sitecat_worker as worker
    for nsites in (257, 1000):
        free = worker.run(product, states, rate_cats, nsites)
        out = tmp_path / f"capped_{nsites}.npz"
        env = dict(os.environ, PLLHIP_SITECAT_BLOCKS="1")
        subprocess.run([sys.executable, os.path.join(HERE, "_sitecat_worker.py"), str(states), str(rate_cats),
                        str(nsites), str(out)], env=env, check=True, timeout=120)
        capped = np.load(out)
        assert set(capped.files) == set(free)
        for name in free:
            if name.endswith("_1"):                     # the second of two runs: the same bits as the first
                assert np.array_equal(free[name], free[name[:-1] + "0"], equal_nan=True), name
                assert np.array_equal(capped[name], capped[name[:-1] + "0"], equal_nan=True), name
            elif not name.endswith("_0"):
                assert np.array_equal(free[name], capped[name]), (nsites, name)
            else:                                       # sums: another grid, another order of summation
                assert np.allclose(free[name], capped[name], rtol=1e-12, atol=0, equal_nan=True), (nsites, name)


# ---------------------------------------------------------------------------
# pllhip_sitecat_from_table
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cats", [1, 2, 4, 9])
@pytest.mark.parametrize("sites", [1, 255, 256, 257, 1000])
def test_disjoint_classes_are_counted_exactly(product, sites, cats):
    """g[n][r] = 1 iff site n is of class r: one iteration gives w_r = M_r / M exactly, the second changes nothing"""
    cls = (pc.splitmix64(7 + sites, sites) % np.uint64(cats)).astype(np.int64)
    m = (pc.splitmix64(11 + cats, sites) % np.uint64(5)).astype(np.uint32) + np.uint32(sites == 1)
    g = np.zeros((sites, cats))
    g[np.arange(sites), cls] = 1.0
    present = np.array([m[cls == r].sum() for r in range(cats)], dtype=np.float64)
    start = np.arange(1.0, cats + 1.0)
    for weights in (m, None):
        M = present if weights is not None else np.bincount(cls, minlength=cats).astype(np.float64)
        if M.sum() == 0:
            continue
        with pc.SiteCat.from_table(product, g, weights, start / start.sum()) as sc:
            one, two = sc.em_weights(0.0, 1), sc.em_weights(0.0, 2)
            assert np.array_equal(one.weights, M / M.sum()) and one.iterations == 1
            assert np.array_equal(two.weights, one.weights)
            po = sc.posteriors(one.weights, FULL)
            assert po.rate is None and po.invariant_prob is None
            live = one.weights[cls] > 0                  # (a class of sites without weight has none itself: T = 0 there)
            assert np.array_equal(po.posterior[live], g[live]) and not po.posterior[~live].any()
            assert np.array_equal(po.category[live], cls.astype(np.uint8)[live])
            assert np.array_equal(po.expected, M)


@pytest.mark.gpu
@pytest.mark.parametrize("cats", [2, 9])
@pytest.mark.parametrize("sites", [1, 255, 256, 257, 1000])
def test_random_table_step_by_step(product, sites, cats):
    g = pc.uniform01(5 + sites, sites * cats).reshape(sites, cats) ** 8
    m = (pc.splitmix64(3 + sites, sites) % np.uint64(4)).astype(np.uint32) + np.uint32(1)
    tab = sr.Table()
    tab.A, tab.B, tab.c = g.astype(LD), np.zeros_like(g, dtype=LD), np.zeros(sites, dtype=np.int64)
    with pc.SiteCat.from_table(product, g, m) as sc:
        a, b, c = sc.table()
        assert np.array_equal(a, g) and not b.any() and not c.any()
        fit = sc.em_weights(1e-9, 6)
        assert np.array_equal(fit.trail_weights[0], np.full(cats, 1.0 / cats))
        # (S = 0: no state sums stand behind an entry that came from the host)
        check_trail(fit, tab, m, 0, cats, sites)
        po = sc.posteriors(fit.weights, FULL)
    inst = type("Shape", (), {"S": 0, "R": cats})
    Tally().check(inst, tab, po, f"{sites} x {cats}", fit.weights, m, None, with_rates=False)


# ---------------------------------------------------------------------------
# what is refused
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(product):
    L = product.lib
    INVALID = 113                                          # PLL_ERROR_PARAM_INVALID

    def refused(call):
        product.errno = 0
        with pytest.raises(RuntimeError):
            call()
        assert product.errno == INVALID, product.errmsg

    with build_case(product, 4, 4, 33, True) as inst:
        t = inst.tree
        edge = (t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix)
        assert not L.pllhip_sitecat_edge(None, *edge, inst.params_p) and product.errno == INVALID
        assert not L.pllhip_sitecat_edge(inst.p, *edge, None) and product.errno == INVALID
        refused(lambda: pc.SiteCat.edge(inst, 99, *edge[1:]))
        refused(lambda: pc.SiteCat.edge(inst, edge[0], 99, *edge[2:]))
        refused(lambda: pc.SiteCat.edge(inst, *edge[:2], 99, *edge[3:]))
        refused(lambda: pc.SiteCat.edge(inst, *edge[:4], 99))
        refused(lambda: pc.SiteCat.edge(inst, *edge, params=[0, 0, 7, 0]))
        with pc.SiteCat.edge(inst, *edge) as sc:
            refused(lambda: sc.posteriors([0.5, -0.1, 0.3, 0.3]))
            refused(lambda: sc.posteriors([0.5, np.nan, 0.3, 0.3]))
            refused(lambda: sc.posteriors([0.0, 0.0, 0.0, 0.0]))
            refused(lambda: sc.posteriors(flags=2))
            refused(lambda: sc.em_weights(1e-3, 5, start=[np.inf, 0.1, 0.1, 0.1]))
    assert L.pllhip_set_sharding(2, None)
    try:
        shard = build_case(product, 20, 4, 161, True)
    finally:
        assert L.pllhip_set_sharding(0, None)
    with shard:
        t = shard.tree
        refused(lambda: pc.SiteCat.edge(shard, t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix))
    with build_case(product, 4, 4, 33, True, attributes=pc.PLL_ATTRIB_AB_FLAG | pc.PLL_ATTRIB_AB_LEWIS) as asc:
        asc.set_asc(pc.PLL_ATTRIB_AB_LEWIS)
        pc.full_traversal(asc)
        t = asc.tree
        with pc.SiteCat.edge(asc, t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix) as sc:
            assert sc.sites == 33 and sc.posteriors(flags=FULL).posterior.shape == (33, 4)   # allowed, uncorrected
            refused(lambda: sc.em_weights(1e-3, 5))
    g = np.ones((5, 3))
    refused(lambda: pc.SiteCat.from_table(product, np.ones((2, 257))))
    for bad in (-1.0, np.nan, np.inf):
        h = g.copy()
        h[3, 1] = bad
        refused(lambda: pc.SiteCat.from_table(product, h))
    refused(lambda: pc.SiteCat.from_table(product, g, None, [0.5, -0.5, 1.0]))
    refused(lambda: pc.SiteCat.from_table(product, g, None, [0.0, 0.0, 0.0]))
    h = g.copy()
    h[2] = 0.0                                             # a site with a pattern weight and no likelihood
    with pc.SiteCat.from_table(product, h) as sc:
        product.errno = 0
        with pytest.raises(RuntimeError, match="site 2 "):
            sc.em_weights(1e-3, 5)
        assert product.errno == INVALID
        assert sc.posteriors().loglh == -np.inf and not sc.posteriors(flags=FULL).posterior[2].any()
    with pc.SiteCat.from_table(product, h, [1, 1, 0, 1, 1]) as sc:    # ... but not with weight 0
        assert np.isfinite(sc.em_weights(1e-3, 5).loglh)
