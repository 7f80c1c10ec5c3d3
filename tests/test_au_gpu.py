"""Multiscale bootstrap replicates and the AU test on the device (pllhip_sitelh_au, pllhip_multiscale_weights) against
the host restatement tests/au_reference.py; shapes, inputs and references: tests/au_cases.py.

Bounds.  Counts: exact.  Replicates: |R - R_ref| <= 2 (S + 4) 2^-53 sum_s C|L|, the bound of the contract
(tests/test_rell_gpu.py derives it).  Proportions: the reference decides every (scale, replicate) row in long double
from its own counts and calls a row undecided when its margin is within 4 x the largest such bound; a device count has
to lie in [certain, certain + undecided], and at most 1 % of a shape's rows may be undecided (none is, see
test_au_reference.py).  Fit: the long-double reference applied to the device's own bp_count, within
au_cases.FIT_TOLERANCE = 16 x the largest float64 / long-double difference of the reference itself over the shapes
(p_au 2.2e-12, d 2.9e-12, c 2.6e-12, se 3.5e-12, rss 4.3e-13); `used` exactly."""
import numpy as np
import pytest

import au_cases as ac
import au_reference as ar
import pllhip_ctypes as pc
import rell_reference as rr

pytestmark = pytest.mark.gpu

LD = np.longdouble
SEED = ac.SEED
FLAG = pc.PLLHIP_AU_REPLICATES
BASE = (257, 5, 100, 10, "mixed", "noisy")
FIT_FIELDS = ("p_au", "d", "c", "se", "rss")


def filled_set(product, S, L, w):
    sl = pc.SiteLikelihoods(product, S, w)
    assert sl.h, product.errmsg
    for t in range(len(L)):
        assert sl.add(L[t]) == t, product.errmsg
    return sl


def set_of(product, shape):
    S, T, _, _, kind, rows = shape
    return filled_set(product, S, ac.rows_of(S, T, kind, rows), ac.weights_of(S, kind))


_runs = {}


def run(product, shape):
    """the device result of a shape with the replicate matrix, computed once"""
    if shape not in _runs:
        with set_of(product, shape) as sl:
            got = sl.au(shape[2], SEED, ac.scales_of(shape[3]), FLAG)
            assert got is not None, product.errmsg
        _runs[shape] = got
    return _runs[shape]


def same_result(a, b, replicates=True):
    return ((not replicates or a.R.tobytes() == b.R.tobytes()) and a.lnl.tobytes() == b.lnl.tobytes() and
            a.best == b.best and np.array_equal(a.draws, b.draws) and np.array_equal(a.bp_count, b.bp_count) and
            np.array_equal(a.used, b.used) and all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in FIT_FIELDS))


# ---------------------------------------------------------------------------
# 1. counts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("S", ac.S_SWEEP)
def test_multiscale_weights_are_the_reference_counts(product, S):
    w = ac.weights_of(S, "mixed", 70000)
    N = int(w.astype(np.int64).sum())
    K = 10
    for k in (0, K - 1):
        n_k = ar.draws_of(ar.DEFAULT_SCALES[k], N)
        got = pc.multiscale_weights(product, w, S, SEED, k, n_k, 0, 6)
        assert got is not None, product.errmsg
        want = ar.counts(w, SEED, k, n_k, 0, 6)
        assert np.array_equal(got, want) and (got.sum(axis=1) == n_k).all()
        window = pc.multiscale_weights(product, w, S, SEED, k, n_k, 37, 3)
        assert np.array_equal(window, ar.counts(w, SEED, k, n_k, 37, 3))
    assert got.max() > 65535
    # N draws of a scale's stream are not the bootstrap replicate
    same_length = pc.multiscale_weights(product, w, S, SEED, 5, N, 0, 2)
    assert np.array_equal(same_length, ar.counts(w, SEED, 5, N, 0, 2))
    plain = pc.bootstrap_weights(product, w, S, SEED, 0, 2)
    assert plain.sum() == same_length.sum() == 2 * N
    assert S == 1 or not np.array_equal(same_length, plain)


def test_multiscale_weights_with_unit_weights(product):
    S = 300
    got = pc.multiscale_weights(product, None, S, 9, 3, 411, 2, 3)
    assert np.array_equal(got, ar.counts(np.ones(S, np.int64), 9, 3, 411, 2, 3))
    assert np.array_equal(pc.multiscale_weights(product, np.ones(S, np.uint32), S, 9, 3, 411, 2, 3), got)
    assert not np.array_equal(pc.multiscale_weights(product, None, S, 9, 4, 411, 2, 3), got)


# ---------------------------------------------------------------------------
# 2. replicates
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ac.SHAPES, ids=ac.shape_id)
def test_replicates_within_the_derived_bound(product, shape):
    S, T, B, K, _, _ = shape
    got, ref = run(product, shape), ac.reference_of(shape)
    assert (got.trees, got.replicates, got.scales) == (T, B, K) and got.R.shape == (K, B, T)
    assert got.draws.tolist() == ref.draws
    err_R = np.abs(got.R.astype(LD) - ref.R)
    err_lnl = np.abs(got.lnl.astype(LD) - ref.lnl)
    print(f"{ac.shape_id(shape)}: worst |R - ref| {float(err_R.max()):.3g} (bound {float(ref.bound.max()):.3g}), "
          f"worst ratio {float((err_R / ref.bound).max()):.3g}; lnl {float(err_lnl.max()):.3g}")
    assert (err_R <= ref.bound).all()
    assert (err_lnl <= ref.bound_lnl).all()
    assert got.best == int(np.argmax(got.lnl))


# ---------------------------------------------------------------------------
# 3. proportions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ac.SHAPES, ids=ac.shape_id)
def test_proportions_between_the_certain_and_the_undecided(product, shape):
    S, T, B, K, _, _ = shape
    got, ref = run(product, shape), ac.reference_of(shape)
    print(f"{ac.shape_id(shape)}: tolerance {float(ref.tol):.3g}, undecided rows {int(ref.undecided.sum())}")
    assert ref.undecided.sum() <= 0.01 * K * B, f"inconclusive: {ref.undecided.sum()} of {K * B} rows undecided"
    assert (ref.certain <= got.bp_count).all() and (got.bp_count <= ref.certain + ref.undecided).all()
    assert (got.bp_count.sum(axis=1) == B).all()
    # the same numbers when the rows of R are consumed pass by pass and dropped
    with set_of(product, shape) as sl:
        lean = sl.au(B, SEED, ac.scales_of(K))
    assert lean is not None and lean.R is None and same_result(got, lean, replicates=False)


# ---------------------------------------------------------------------------
# 4. fit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ac.SHAPES, ids=ac.shape_id)
def test_fit_against_the_long_double_reference(product, shape):
    S, T, B, K, _, _ = shape
    got, ref = run(product, shape), ac.reference_of(shape)
    want = ar.fit(got.bp_count, B, ref.rho, ref.kstar)
    assert got.used.tolist() == want.used.tolist()
    for name in FIT_FIELDS:
        err = float(np.abs(getattr(got, name).astype(LD) - getattr(want, name)).max())
        print(f"{ac.shape_id(shape)}: worst |{name} - ref| {err:.3g} (tolerance {ac.FIT_TOLERANCE[name]:.3g})")
    for name in FIT_FIELDS:
        assert (np.abs(getattr(got, name).astype(LD) - getattr(want, name)) <= ac.FIT_TOLERANCE[name]).all(), name
    assert ((got.p_au >= 0) & (got.p_au <= 1)).all()


def test_fitted_and_degenerate_trees_together(product):
    got, ref = run(product, ac.RANKED), ac.reference_of(ac.RANKED)
    assert (got.used[:3] >= 3).all() and got.used[3] == 0
    assert got.best == 0 and got.p_au[0] > got.p_au[1] > got.p_au[2] > 0
    assert got.p_au[3] == 0 and got.d[3] == got.c[3] == got.se[3] == got.rss[3] == 0
    assert (got.se[:3] > 0).all() and (got.rss[:3] > 0).all()
    assert not np.array_equal(got.bp_count[ref.kstar, :3] / 100.0, got.p_au[:3])


# ---------------------------------------------------------------------------
# 5. independence
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [BASE, (3 * ac.CHUNK + 5, 5, 100, 10, "mixed", "noisy"),
                                   (257, 33, 100, 10, "mixed", "noisy"), (257, 5, 48, 64, "mixed", "noisy")],
                         ids=ac.shape_id)
def test_results_do_not_depend_on_the_batch_or_the_run(product, shape):
    S, T, B, K, _, _ = shape
    first = run(product, shape)
    with set_of(product, shape) as sl:
        for batch in (16, 48, 0, 0):
            again = sl.au(B, SEED, ac.scales_of(K), FLAG, batch=batch)
            assert again is not None, product.errmsg
            assert batch == 0 or again.batch == batch
            assert same_result(first, again), batch
        other_seed = sl.au(B, SEED + 1, ac.scales_of(K), FLAG)
        assert other_seed.R.tobytes() != first.R.tobytes()


def test_a_scale_does_not_depend_on_the_other_scales_or_on_B(product):
    S, T, B, K, _, _ = BASE
    whole = run(product, BASE)
    scales = list(ar.DEFAULT_SCALES)
    with set_of(product, BASE) as sl:
        # a scale keeps its stream with its index: drop the last scales, or grow B
        fewer = sl.au(B, SEED, scales[:4], FLAG)
        assert fewer.scales == 4 and fewer.R.tobytes() == whole.R[:4].tobytes()
        assert np.array_equal(fewer.bp_count, whole.bp_count[:4]) and np.array_equal(fewer.draws, whole.draws[:4])
        more = sl.au(B + 37, SEED, None, FLAG)
        assert more.R[:, :B].tobytes() == whole.R.tobytes()
        # another scale in place of scale 2 leaves the others alone
        swapped = sl.au(B, SEED, scales[:2] + [0.75] + scales[3:], FLAG)
        keep = [k for k in range(K) if k != 2]
        assert swapped.R[keep].tobytes() == whole.R[keep].tobytes()
        assert np.array_equal(swapped.bp_count[keep], whole.bp_count[keep])
        assert swapped.R[2].tobytes() != whole.R[2].tobytes()


@pytest.mark.parametrize("S", [257, 3 * ac.CHUNK + 5])
def test_equal_rows_give_equal_columns(product, S):
    L = ac.rows_of(S, 5, "mixed", "noisy").copy()
    L[4] = L[2]
    w = ac.weights_of(S, "mixed")
    with filled_set(product, S, L, w) as sl:
        got = sl.au(100, SEED, None, FLAG)
    assert got.R[:, :, 4].tobytes() == got.R[:, :, 2].tobytes() and got.lnl[4].tobytes() == got.lnl[2].tobytes()
    assert (got.bp_count[:, 4] == 0).all()
    # two equal rows alone: every win goes to the lower index, and no scale is usable
    with filled_set(product, S, L[[2, 4]], w) as sl:
        got = sl.au(100, SEED, None, FLAG)
    assert (got.bp_count == [100, 0]).all() and got.used.tolist() == [0, 0]
    assert got.p_au.tolist() == [1.0, 0.0] and not (got.d.any() or got.c.any() or got.se.any() or got.rss.any())
    # 17 equal rows: the copies sit in another tile and in another column than the original
    with filled_set(product, S, np.vstack([L[:4], np.repeat(L[2:3], 17, axis=0)]), w) as sl:
        got = sl.au(20, SEED, None, FLAG)
    assert all(got.R[:, :, t].tobytes() == got.R[:, :, 2].tobytes() for t in range(4, 21))


# ---------------------------------------------------------------------------
# 6. rows written on the device
# ---------------------------------------------------------------------------
def test_rows_from_the_edge_path(product):
    sites = (130, 257)
    S = sum(sites)
    w = np.random.default_rng(5).integers(0, 4, S).astype(np.uint32)
    a = pc.build_instance(product, states=4, rate_cats=4, ntips=12, nsites=sites[0])
    b = pc.build_instance(product, states=20, rate_cats=4, ntips=12, nsites=sites[1])
    with a, b, pc.SiteLikelihoods(product, S, w) as dev, pc.SiteLikelihoods(product, S, w) as host:
        for tree, (edge, factor) in enumerate(((a.tree.nedges - 1, 1.0), (0, 1.7), (5, 0.4))):
            want = np.zeros(S)
            for inst, offset in ((a, 0), (b, sites[0])):
                t = inst.tree
                t.set_root_edge(edge)
                t.brlens[edge] *= factor
                pc.full_traversal(inst)
                args = (t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix)
                _, persite = inst.edge_lnl(*args, persite=True)
                assert dev.add_edge(tree, offset, inst, *args) is not None, product.errmsg
                want[offset:offset + inst.N] = persite
            assert dev.get(tree).tobytes() == want.tobytes()
            assert host.add(want) == tree
        got_dev, got_host = dev.au(200, SEED, None, FLAG), host.au(200, SEED, None, FLAG)
        assert got_dev is not None and got_host is not None, product.errmsg
        assert same_result(got_dev, got_host)
        assert len(set(got_dev.lnl)) == 3 and got_dev.p_au.max() > 0


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_refusals(product):
    S = 40
    inst = pc.build_instance(product, states=4, rate_cats=4, ntips=12, nsites=30)
    with inst, pc.SiteLikelihoods(product, S, None) as sl:
        pc.full_traversal(inst)
        calls = inst.counters().lnl_calls

        def refused(value, code=pc.PLL_ERROR_PARAM_INVALID):
            assert value is None and product.errno == code, (value, product.errno, product.errmsg)
            assert product.errmsg
            product.errno = 0

        product.errno = 0
        assert ar.refusal(None, S, 10, 0) == "empty"
        refused(sl.au(10, SEED))                                         # the set is empty
        assert sl.add(np.linspace(-5.0, -1.0, S)) == 0 and sl.add(np.linspace(-4.0, -2.0, S)) == 1
        good = sl.au(10, SEED)
        assert good is not None and good.draws.tolist() == [20, 24, 28, 32, 36, 40, 44, 48, 52, 56]
        cases = [(0, None), (1 << 24, None),                             # B = 0, B >= 2^24
                 (10, [1.0]), (10, list(np.linspace(0.5, 1.4, 65))),                 # K < 2, K > 64
                 (10, [1.0, np.nan]), (10, [1.0, np.inf]), (10, [1.0, -np.inf]), (10, [0.0, 1.0]), (10, [1.0, -0.5]),
                 (10, [1.0, 0.01]),                                      # n_k = 0
                 (10, [1.0, 2.0 ** 40 / S]),                             # n_k = 2^40
                 (10, [1.0, 1.3, 1.004]),                                # scales 0 and 2 both draw 40
                 (10, [0.5, 0.51])]                                      # both 20 (0.51 * 40 + 0.5 = 20.9)
        for B, scale in cases:
            assert ar.refusal(scale, S, B, 2) is not None, (B, scale)
            refused(sl.au(B, SEED, scale))
        assert ar.refusal([1.0, (2.0 ** 40 - 1) / S], S, 10, 2) is None
        refused(sl.au(10, SEED, [0.5, 1.0], scales=1))                   # K counts, not the array behind it
        assert sl.au(10, SEED, [0.5, 1.0, 1.0], scales=2) is not None    # ... and the third value is never read
        ignored = sl.au(10, SEED, None, scales=1)                        # scale == NULL: `scales` is ignored
        assert ignored is not None and ignored.scales == 10
        refused(pc.multiscale_weights(product, None, 10, 1, 64, 10, 0, 1))           # scale index
        refused(pc.multiscale_weights(product, None, 10, 1, 0, 0, 0, 1))             # no draw
        refused(pc.multiscale_weights(product, None, 10, 1, 0, 1 << 40, 0, 1))
        refused(pc.multiscale_weights(product, None, 10, 1, 0, 10, (1 << 24) - 1, 1))
        refused(pc.multiscale_weights(product, np.zeros(4, np.uint32), 4, 1, 0, 10, 0, 1))
        assert inst.counters().lnl_calls == calls


def test_a_single_tree_wins_everything(product):
    got = run(product, (257, 1, 100, 10, "mixed", "noisy"))
    assert (got.bp_count == 100).all() and got.best == 0
    assert got.p_au.tolist() == [1.0] and got.used.tolist() == [0]
    assert got.d[0] == got.c[0] == got.se[0] == got.rss[0] == 0


def test_a_device_written_minus_infinity_is_named(product):
    """three tips, zero-length matrices between tips 0 and 1: a site where they differ has likelihood 0"""
    n, offset = 64, 3
    tree = pc.Tree(3, 42, 43)
    tree.brlens[:] = [0.0, 0.0, 0.1]
    inst = pc.build_instance(product, states=4, rate_cats=4, ntips=3, nsites=n, tree=tree)
    inner = tree.root_a
    kids = [v for (v, _) in tree.adj[inner] if v != tree.root_b]
    differ = np.flatnonzero(inst.codes[kids[0]] != inst.codes[kids[1]])
    assert len(differ) and tree.brlens[tree.root_matrix] > 0
    with inst, pc.SiteLikelihoods(product, n + 5, None) as sl:
        pc.full_traversal(inst)
        assert sl.add(np.full(n + 5, -2.0)) == 0
        ok = sl.au(10, SEED)
        assert ok is not None and (ok.bp_count[:, 0] == 10).all()
        args = (tree.root_a, tree.scaler_of(tree.root_a), tree.root_b, tree.scaler_of(tree.root_b), tree.root_matrix)
        lnl = sl.add_edge(1, offset, inst, *args)
        assert lnl == -np.inf and sl.count == 2
        product.errno = 0
        assert sl.au(10, SEED) is None
        assert product.errno != 0
        assert "pllhip_sitelh_au" in product.errmsg and f"row 1 at pattern {offset + differ[0]}" in product.errmsg
