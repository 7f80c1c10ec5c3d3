"""The host restatement of the resampling definitions (tests/rell_reference.py) against known answers, a plain
Python-integer loop and the properties every correct implementation has.  No GPU."""
import numpy as np
import pytest

import rell_reference as rr

LD = np.longdouble


def heavy_weights(S, seed):
    """weights 0 .. 3, zeros included, and one pattern of weight 70000"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 4, S).astype(np.int64)
    if S > 3:
        w[1] = 0
    w[S // 2] = 70000
    return w


@pytest.fixture(scope="module")
def thousand():
    """C[1000][257] for seed 7"""
    w = heavy_weights(257, 11)
    return w, rr.counts(w, 7, 0, 1000)


def test_known_answers():
    assert int(rr.mix(0, 0)) == 0xE220A8397B1DCDAF
    assert int(rr.mix(0, 1)) == 0x6E789E6AA1B965F4
    u = rr.mix(42, (3 << 40) | 7)
    assert int(u) == 0x45672D2D0BAF0B73
    assert int(rr.mulhi64(u, 70401)) == 19086
    assert int(rr.sites_of(42, 3, 70401)[7]) == 19086


def test_mulhi64_against_python_integers():
    u = rr.mix(5, np.arange(2000))
    for n in (1, 3, 70401, (1 << 32) - 1, 1 << 32, (1 << 40) - 1):
        want = [(int(x) * n) >> 64 for x in u]
        assert [int(x) for x in rr.mulhi64(u, n)] == want


def test_draws_against_a_plain_integer_loop():
    w = [2, 0, 1, 5, 0, 3, 1]
    for seed, first in ((0, 0), (42, 3), (2**64 - 1, (1 << 24) - 3)):
        assert np.array_equal(rr.counts(w, seed, first, 3), rr.counts_brute_force(w, seed, first, 3))
    assert np.array_equal(rr.counts([4], 9, 0, 2), [[4], [4]])


def test_every_replicate_draws_n_sites(thousand):
    w, C = thousand
    assert (C.sum(axis=1) == w.sum()).all()
    assert not C[:, w == 0].any()
    assert C.max() > 65535                      # the counts of the heavy pattern do not fit 16 bits


def test_count_means_match_the_weights(thousand):
    """C[b][s] is Binomial(N, w_s / N): over 1000 replicates its mean stays within 5 standard errors of w_s"""
    w, C = thousand
    n = w.sum()
    p = w / n
    se = np.sqrt(n * p * (1 - p) / C.shape[0])
    z = np.abs(C.mean(axis=0) - w)[w > 0] / se[w > 0]
    print(f"worst pattern: {z.max():.2f} standard errors")
    assert z.max() < 5.0


def example(S=64, T=4, B=200, seed=3):
    rng = np.random.default_rng(seed)
    w = heavy_weights(S, seed)
    base = -rng.gamma(2.0, 4.0, S)
    L = base[None, :] + 0.3 * rng.standard_normal((T, S))
    C = rr.counts(w, seed, 0, B)
    return w, L, C


def test_a_tree_better_at_every_site_wins_every_replicate():
    w, L, C = example()
    L[2] = L.max(axis=0) + 0.01
    st = rr.statistics(rr.replicates(C, L), rr.replicates(w[None, :], L)[0])
    B = C.shape[0]
    assert st.best == 2 and st.bp_count[2] == B and st.bp_count.sum() == B
    assert st.elw[2] > 0.5


@pytest.mark.parametrize("S,T,B", [(64, 4, 200), (5, 1, 17), (257, 17, 50), (1, 3, 10)])
def test_invariants(S, T, B):
    w, L, C = example(S, T, B, seed=S + T)
    R, lnl = rr.replicates(C, L), rr.replicates(w[None, :], L)[0]
    st = rr.statistics(R, lnl)
    assert st.best == int(np.argmax(lnl))
    assert st.bp_count.sum() == B
    assert abs(st.elw.sum() - 1) < 1e-12
    assert st.kh_count[st.best] == B and st.sh_count[st.best] == B
    for c in (st.bp_count, st.kh_count, st.sh_count):
        assert (c >= 0).all() and (c <= B).all()
    # with no tolerance nothing but exact ties is undecided, and certain + undecided covers every count
    d = rr.decided(R, lnl, LD(0))
    other = np.arange(T) != st.best
    for (certain, undecided), c in ((d.bp, st.bp_count), (d.kh, st.kh_count), (d.sh, st.sh_count)):
        assert (certain[other] <= c[other]).all() and (c[other] <= (certain + undecided)[other]).all()


def test_equal_rows_tie_to_the_lowest_index():
    w, L, C = example(T=5)
    L[4] = L[2]
    st = rr.statistics(rr.replicates(C, L), rr.replicates(w[None, :], L)[0])
    assert st.bp_count[4] == 0
