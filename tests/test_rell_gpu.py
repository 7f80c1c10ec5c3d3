"""Site-likelihood sets, RELL resampling with the KH / SH / ELW statistics and bootstrap weights on the device, against
the host restatement tests/rell_reference.py.

Bounds.  An fp64 sum of S rounded products, in any order, differs from the exact sum by at most
(S + 4) 2^-53 sum |terms| (to first order; the factor 2 below covers the higher orders and the long-double reference's
own error), so every replicate log-likelihood has to satisfy |R - R_ref| <= 2 (S + 4) 2^-53 sum_s C[b][s] |L[t][s]|.
The counts are decisions: the reference recomputes each in long double from the device's own R and calls it
undecided when its margin is within 4 x the largest such bound; a device count has to lie in
[certain, certain + undecided].  ELW: 1e-9 (the error of exp, 2^-52 per term over at most 33 terms, with a wide
margin)."""
import functools

import numpy as np
import pytest

import pllhip_ctypes as pc
import rell_reference as rr

pytestmark = pytest.mark.gpu

LD = np.longdouble
SEED = 0x5EED0000BEEF
FLAG = pc.PLLHIP_RELL_REPLICATES
CHUNK = 1024            # patterns per partial sum up to 65536 patterns
S_SWEEP = [1, 3, 4, 5, 63, 64, 65, 257, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5]
T_SWEEP = [1, 2, 15, 16, 17, 33]
B_SWEEP = [1, 15, 16, 17, 1000]
SHAPES = [(S, 5, 100) for S in S_SWEEP] + [(257, T, 100) for T in T_SWEEP] + [(257, 5, B) for B in B_SWEEP]
SHAPES.append((65, 130, 17))        # more trees than a wave carries in one pass (128): a second group of tree tiles


# ---------------------------------------------------------------------------
# inputs and references, computed once
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights_of(S):
    """weights 0 .. 3, zeros included, one pattern of weight 70000"""
    rng = np.random.default_rng(1000 + S)
    w = rng.integers(0, 4, S).astype(np.uint32)
    if S > 3:
        w[1] = 0
    w[S // 2] = 70000
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def rows_of(S, T):
    """L[t][s] = base_s + noise: base_s = -Gamma(2, 4), sigma 0.3 (1e-4 at the heavy pattern), one value -1e4"""
    rng = np.random.default_rng(2000 + 7 * S + T)
    base = -rng.gamma(2.0, 4.0, S)
    sigma = np.full(S, 0.3)
    sigma[S // 2] = 1e-4
    L = base[None, :] + sigma[None, :] * rng.standard_normal((T, S))
    L[T - 1, S - 1] = -1e4
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def all_counts(S):
    """the reference's C for the replicates any shape with this S asks for"""
    B = max(b for (s, _, b) in SHAPES if s == S)
    C = rr.counts(weights_of(S), SEED, 0, B)
    C.setflags(write=False)
    return C


def filled_set(product, S, L, w):
    sl = pc.SiteLikelihoods(product, S, w)
    assert sl.h, product.errmsg
    for t in range(len(L)):
        assert sl.add(L[t]) == t, product.errmsg
    return sl


_runs = {}


def run(product, shape):
    """(device result with the replicate matrix, reference C) of a shape, computed once"""
    if shape not in _runs:
        S, T, B = shape
        with filled_set(product, S, rows_of(S, T), weights_of(S)) as sl:
            assert sl.count == T
            got = sl.rell(B, SEED, FLAG)
            assert got is not None, product.errmsg
        _runs[shape] = (got, all_counts(S)[:B])
    return _runs[shape]


def bounds(shape, C):
    """(bound of R [B][T], bound of lnl [T])"""
    S, T, _ = shape
    L, w = rows_of(S, T), weights_of(S)
    unit = LD(2 * (S + 4)) * LD(2) ** -53
    return unit * rr.magnitudes(C, L), unit * rr.magnitudes(w[None, :], L)[0]


def same_result(a, b):
    return (a.R.tobytes() == b.R.tobytes() and a.lnl.tobytes() == b.lnl.tobytes() and a.best == b.best and
            a.elw.tobytes() == b.elw.tobytes() and np.array_equal(a.bp_count, b.bp_count) and
            np.array_equal(a.kh_count, b.kh_count) and np.array_equal(a.sh_count, b.sh_count))


# ---------------------------------------------------------------------------
# 1. weights
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("S", S_SWEEP)
def test_bootstrap_weights_are_the_reference_counts(product, S):
    C = all_counts(S)
    w = weights_of(S)
    got = pc.bootstrap_weights(product, w, S, SEED, 0, 20)
    assert got is not None, product.errmsg
    assert np.array_equal(got, C[:20])
    window = pc.bootstrap_weights(product, w, S, SEED, 37, 5)
    assert np.array_equal(window, C[37:42])
    assert got.max() > 65535


def test_bootstrap_weights_with_unit_weights(product):
    S = 300
    got = pc.bootstrap_weights(product, None, S, 9, 2, 3)
    assert np.array_equal(got, rr.counts(np.ones(S, np.int64), 9, 2, 3))
    assert np.array_equal(pc.bootstrap_weights(product, np.ones(S, np.uint32), S, 9, 2, 3), got)


# ---------------------------------------------------------------------------
# 2. replicates
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "S%d-T%d-B%d" % s)
def test_replicates_within_the_derived_bound(product, shape):
    S, T, B = shape
    got, C = run(product, shape)
    L, w = rows_of(S, T), weights_of(S)
    bound_R, bound_lnl = bounds(shape, C)
    err_R = np.abs(got.R.astype(LD) - rr.replicates(C, L))
    err_lnl = np.abs(got.lnl.astype(LD) - rr.replicates(w[None, :], L)[0])
    print(f"{shape}: worst |R - ref| {float(err_R.max()):.3g} (bound {float(bound_R.max()):.3g}), "
          f"worst ratio {float((err_R / bound_R).max()):.3g}; lnl {float(err_lnl.max()):.3g}")
    assert got.R.shape == (B, T) and got.trees == T and got.replicates == B
    assert (err_R <= bound_R).all()
    assert (err_lnl <= bound_lnl).all()


# ---------------------------------------------------------------------------
# 3. counts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "S%d-T%d-B%d" % s)
def test_counts_and_weights_from_the_device_replicates(product, shape):
    S, T, B = shape
    got, C = run(product, shape)
    bound_R, bound_lnl = bounds(shape, C)
    tol = 4 * max(bound_R.max(), bound_lnl.max())
    ref = rr.decided(got.R, got.lnl, tol)
    assert got.best == ref.best == int(np.argmax(got.lnl))
    other = np.arange(T) != ref.best
    print(f"{shape}: tolerance {float(tol):.3g}, undecided bp {ref.bp[1].sum()} kh {ref.kh[1][other].sum()} "
          f"sh {ref.sh[1][other].sum()}")
    for name, (certain, undecided), count in (("bp", ref.bp, got.bp_count), ("kh", ref.kh, got.kh_count),
                                              ("sh", ref.sh, got.sh_count)):
        assert (undecided[other] <= 0.01 * B).all(), f"inconclusive: {name} leaves {undecided} of {B} undecided"
        low, high = certain, certain + undecided
        if name != "bp":
            low, high = low[other], high[other]
            count = count[other]
        assert (low <= count).all() and (count <= high).all(), (name, certain, undecided, count)
    assert got.bp_count.sum() == B
    assert got.kh_count[ref.best] == B and got.sh_count[ref.best] == B
    err = np.abs(got.elw.astype(LD) - ref.elw)
    print(f"{shape}: worst |elw - ref| {float(err.max()):.3g}")
    assert (err <= 1e-9).all()
    assert abs(got.elw.sum() - 1) < 1e-12


# ---------------------------------------------------------------------------
# 4. reproducibility
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(257, 5, 100), (3 * CHUNK + 5, 5, 100), (257, 33, 100), (257, 5, 1000)],
                         ids=lambda s: "S%d-T%d-B%d" % s)
def test_results_do_not_depend_on_the_batch_or_the_run(product, shape):
    S, T, B = shape
    first, _ = run(product, shape)
    with filled_set(product, S, rows_of(S, T), weights_of(S)) as sl:
        for batch in (16, 48, 0, 0):
            again = sl.rell(B, SEED, FLAG, batch=batch)
            assert again is not None, product.errmsg
            assert batch == 0 or again.batch == min(batch, (B + 15) // 16 * 16)
            assert same_result(first, again), batch
        other_seed = sl.rell(B, SEED + 1, FLAG)
        assert B < 16 or other_seed.R.tobytes() != first.R.tobytes()


@pytest.mark.parametrize("S", [257, 3 * CHUNK + 5])
def test_equal_rows_give_equal_columns(product, S):
    L = rows_of(S, 5).copy()
    L[4] = L[2]
    with filled_set(product, S, L, weights_of(S)) as sl:
        got = sl.rell(100, SEED, FLAG)
    assert got.R[:, 4].tobytes() == got.R[:, 2].tobytes()
    assert got.lnl[4].tobytes() == got.lnl[2].tobytes()
    assert got.bp_count[4] == 0
    assert got.kh_count[4] == got.kh_count[2] and got.sh_count[4] == got.sh_count[2]
    # 17 equal rows: the copies sit in another tile and in another column than the original
    with filled_set(product, S, np.vstack([L[:4], np.repeat(L[2:3], 17, axis=0)]), weights_of(S)) as sl:
        got = sl.rell(100, SEED, FLAG)
    assert all(got.R[:, t].tobytes() == got.R[:, 2].tobytes() for t in range(4, 21))


# ---------------------------------------------------------------------------
# 5. rows written on the device
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
                lnl_ref, persite = inst.edge_lnl(*args, persite=True)
                lnl = dev.add_edge(tree, offset, inst, *args)
                assert lnl is not None, product.errmsg
                assert lnl == lnl_ref and np.isfinite(lnl)
                want[offset:offset + inst.N] = persite
            assert dev.count == tree + 1
            assert dev.get(tree).tobytes() == want.tobytes()
            assert host.add(want) == tree
        # a row may be written again, and a part of it
        t = a.tree
        args = (t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix)
        assert dev.add_edge(2, 0, a, *args) is not None and dev.count == 3
        assert dev.get(2).tobytes() == host.get(2).tobytes()
        got_dev, got_host = dev.rell(200, SEED, FLAG), host.rell(200, SEED, FLAG)
        assert got_dev is not None and got_host is not None, product.errmsg
        assert same_result(got_dev, got_host)
        assert len(set(got_dev.lnl)) == 3


# ---------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------
def test_refusals(product):
    S = 40
    inst = pc.build_instance(product, states=4, rate_cats=4, ntips=12, nsites=30)
    with inst, pc.SiteLikelihoods(product, S, None) as sl:
        pc.full_traversal(inst)
        t = inst.tree
        args = (t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix)
        calls = inst.counters().lnl_calls

        def refused(value, code=pc.PLL_ERROR_PARAM_INVALID):
            assert value is None and product.errno == code, (value, product.errno, product.errmsg)
            product.errno = 0

        product.errno = 0
        refused(sl.rell(10, SEED))                                   # no tree yet
        row = np.linspace(-5.0, -1.0, S)
        for bad in (np.nan, np.inf, -np.inf):
            r = row.copy()
            r[17] = bad
            refused(sl.add(r))
        assert sl.count == 0
        assert sl.add(row) == 0
        refused(sl.rell(0, SEED))                                    # B = 0
        refused(sl.rell(1 << 24, SEED))
        refused(sl.add_edge(2, 0, inst, *args))                      # a row beyond count
        refused(sl.add_edge(1, 11, inst, *args))                     # offset + sites > S
        refused(sl.get(1))
        assert inst.counters().lnl_calls == calls and sl.count == 1
        assert sl.add_edge(1, 10, inst, *args) is not None and sl.count == 2
        assert inst.counters().lnl_calls == calls + 1
    big = pc.SiteLikelihoods(product, 300, np.full(300, 0xFFFFFFFF, np.uint32))      # N >= 2^40
    refused(big.h)
    refused(pc.SiteLikelihoods(product, 4, np.zeros(4, np.uint32)).h)                # N = 0
    refused(pc.SiteLikelihoods(product, 0, None).h)
    refused(pc.bootstrap_weights(product, np.full(300, 0xFFFFFFFF, np.uint32), 300, 1, 0, 1))
    refused(pc.bootstrap_weights(product, None, 10, 1, (1 << 24) - 1, 1))


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
        ok = sl.rell(10, SEED)
        assert ok is not None and ok.bp_count[0] == 10
        args = (tree.root_a, tree.scaler_of(tree.root_a), tree.root_b, tree.scaler_of(tree.root_b), tree.root_matrix)
        lnl = sl.add_edge(1, offset, inst, *args)
        assert lnl == -np.inf and sl.count == 2
        row = sl.get(1)
        assert np.isneginf(row[offset + differ]).all() and np.isfinite(np.delete(row, offset + differ)).all()
        product.errno = 0
        assert sl.rell(10, SEED) is None
        assert product.errno != 0
        assert f"row 1 at pattern {offset + differ[0]}" in product.errmsg, product.errmsg
