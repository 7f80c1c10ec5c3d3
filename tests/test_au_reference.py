"""The host reference of the multiscale bootstrap and the AU test (tests/au_reference.py) against brute force and
against curves it has to recover.  No GPU."""
import math

import numpy as np
import pytest

import au_reference as ar
import rell_reference as rr

LD = np.longdouble
SEED = 0x5EED0000BEEF
WEIGHTS = {
    "unit": lambda S: np.ones(S, np.int64),
    "mixed": lambda S: np.array([(7 * s + 3) % 5 for s in range(S)], np.int64) + (np.arange(S) == S // 2) * 40,
}


# ---------------------------------------------------------------------------
# streams and counts
# ---------------------------------------------------------------------------
def test_known_answers_of_the_scale_streams():
    """the values INTEGRATION.md prints"""
    assert ar.seed_of(0, 0) == 0xE4D971771B652C20
    assert ar.seed_of(0, 1) == 0xE99FF867DBF682C9
    assert ar.seed_of(42, 9) == 0x63C08C484A2D4597
    u = rr.mix(ar.seed_of(42, 9), (3 << 40) | 7)
    assert int(u) == 0x97ED2625D918A690 and int(rr.mulhi64(u, 70401)) == 41780


@pytest.mark.parametrize("S", [1, 5, 63])
@pytest.mark.parametrize("kind", ["unit", "mixed"])
@pytest.mark.parametrize("k", [0, 3])
def test_vectorised_counts_equal_brute_force(S, kind, k):
    w = WEIGHTS[kind](S)
    N = int(w.sum())
    for n_k in (N // 2 if N >= 6 else N + 3, N + 7):
        assert n_k != N
        fast = ar.counts(w, SEED, k, n_k, 2, 4)
        assert np.array_equal(fast, ar.counts_brute_force(w, SEED, k, n_k, 2, 4))
        assert (fast.sum(axis=1) == n_k).all()
        assert (fast[:, w == 0] == 0).all()


def test_scale_streams_differ_and_are_not_the_bootstrap_stream():
    w = WEIGHTS["mixed"](63)
    N = int(w.sum())
    rows = [ar.counts(w, SEED, k, N, 0, 3) for k in range(4)]
    for a in range(4):
        assert not np.array_equal(rows[a], rr.counts(w, SEED, 0, 3))
        for b in range(a):
            assert not np.array_equal(rows[a], rows[b])
    assert len({ar.seed_of(SEED, k) for k in range(64)}) == 64


def test_a_replicate_does_not_depend_on_the_window():
    w = WEIGHTS["mixed"](63)
    whole = ar.counts(w, SEED, 3, 100, 0, 9)
    assert np.array_equal(ar.counts(w, SEED, 3, 100, 5, 2), whole[5:7])
    assert np.array_equal(ar.counts(w, SEED, 3, 100, 8, 1), whole[8:])
    # blocks of the vectorised form: more draws than one block holds
    big = ar.counts(w, SEED, 3, 3_000_000, 1, 3)
    assert np.array_equal(ar.counts(w, SEED, 3, 3_000_000, 2, 1), big[1:2])


# ---------------------------------------------------------------------------
# scales and refusals
# ---------------------------------------------------------------------------
def test_rounding_of_the_draw_counts():
    assert [ar.draws_of(r, 10) for r in ar.DEFAULT_SCALES] == [5, 6, 7, 8, 9, 10, 11, 12, 13, 14]
    assert ar.draws_of(0.5, 5) == 3 and ar.draws_of(0.5, 7) == 4          # halves go up
    assert ar.draws_of(0.25, 5) == 1 and ar.draws_of(0.09, 5) == 0
    assert ar.draws_of(0.7, 257) == math.floor(0.7 * 257.0 + 0.5) == 180
    assert ar.draws_of(float("nan"), 5) is None and ar.draws_of(float("inf"), 5) is None
    assert ar.draws_of(0.0, 5) is None and ar.draws_of(-1.0, 5) is None
    assert ar.ratios([5, 14], 10) == [0.5, 1.4]


def test_every_refusal_predicate():
    ok = dict(scales=None, N=4000, B=100, trees=3)
    assert ar.refusal(**ok) is None
    assert ar.refusal(**{**ok, "B": 0}) == "replicates"
    assert ar.refusal(**{**ok, "B": 1 << 24}) == "replicates"
    assert ar.refusal(**{**ok, "B": (1 << 24) - 1}) is None
    assert ar.refusal(**{**ok, "trees": 0}) == "empty"
    assert ar.refusal(**{**ok, "scales": [1.0]}) == "scales"
    assert ar.refusal(**{**ok, "scales": []}) == "scales"
    assert ar.refusal(**{**ok, "scales": [0.5 + 0.01 * i for i in range(65)]}) == "scales"
    assert ar.refusal(**{**ok, "scales": [0.5 + 0.01 * i for i in range(64)]}) is None
    for bad in (float("nan"), float("inf"), 0.0, -0.5):
        assert ar.refusal(**{**ok, "scales": [1.0, bad]}) == "scale"
    assert ar.refusal(**{**ok, "scales": [1.0, 1e-5]}) == "draws"                    # n_k = 0
    assert ar.refusal(**{**ok, "scales": [1.0, 2.0 ** 40 / 4000]}) == "draws"        # n_k = 2^40
    assert ar.refusal(**{**ok, "scales": [1.0, (2.0 ** 40 - 1) / 4000]}) is None
    assert ar.refusal(**{**ok, "scales": [1.0, 1.0001]}) == "duplicate"              # both 4000
    assert ar.refusal(**{**ok, "N": 5}) == "duplicate"                               # 0.5 and 0.6 of 5 sites
    assert ar.refusal(**{**ok, "N": 1}) == "duplicate"


def test_nearest_scale():
    assert ar.nearest_scale([5, 6, 10, 14], 10) == 2
    assert ar.nearest_scale([9, 11, 30], 10) == 0                  # a tie goes to the lowest k
    assert ar.nearest_scale([30, 20], 10) == 1


# ---------------------------------------------------------------------------
# proportions
# ---------------------------------------------------------------------------
def test_proportions_and_decisions():
    R = np.array([[1.0, 2.0, 2.0], [3.0, 1.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0 + 1e-9, 0.0]])
    assert ar.proportions(R).tolist() == [2, 2, 0]                 # ties to the lowest index
    certain, undecided = ar.decided(R, 1e-6)
    assert certain.tolist() == [1, 0, 0] and undecided.tolist() == [2, 3, 2]
    certain, undecided = ar.decided(R[:, :1], 1e-6)
    assert certain.tolist() == [4] and undecided.tolist() == [0]


# ---------------------------------------------------------------------------
# the fit
# ---------------------------------------------------------------------------
def test_long_double_erfc_and_inverse():
    for x in (0.0, 0.3, 0.999, 1.0, 1.3, 2.2, 4.0, -0.7, -3.0):
        assert abs(float(ar.erfc_ld(x)) / math.erfc(x) - 1) < 4e-16
    # the series and the continued fraction meet
    below, above = ar.erfc_ld(LD(1) - LD(2) ** -40), ar.erfc_ld(LD(1) + LD(2) ** -40)
    slope = 2 / math.sqrt(math.pi) * math.exp(-1.0)
    assert abs(float((below - above) - LD(2) ** -39 * LD(slope))) < 1e-18
    for p in (0.5, 0.3, 1e-3, 1e-8):
        z = ar.upper_tail_inverse_ld(p)
        assert abs(float(ar.erfc_ld(z / ar.SQRT2_LD) / 2 - LD(p))) < 4e-19 * max(p, 1e-3) / 1e-3
        assert abs(ar.upper_tail_inverse_f64(p) - float(z)) < 1e-14
    assert ar.upper_tail_inverse_f64(0.5) == 0.0 or abs(ar.upper_tail_inverse_f64(0.5)) < 1e-16


@pytest.mark.parametrize("d,c", [(1.2, 0.3), (-0.8, 0.5), (2.5, -0.4), (0.1, 0.1)])
@pytest.mark.parametrize("precision", ["float64", "longdouble"])
def test_fit_recovers_a_curve(d, c, precision):
    """proportions exactly on a (d, c) curve, as counts of B = 10^8: rounding a count moves p by at most 5e-9, z by
    that over phi(z) (phi >= 1e-3 here), so d - c by less than 1e-5 x the fit's leverage; asserted: p_au within 1e-6"""
    B = 10 ** 8
    rho = ar.ratios([ar.draws_of(r, 100000) for r in ar.DEFAULT_SCALES], 100000)
    bp = np.zeros((len(rho), 2), np.int64)
    for k, r in enumerate(rho):
        z = d * math.sqrt(r) + c / math.sqrt(r)
        bp[k, 0] = round(float(ar.erfc_ld(LD(z) / ar.SQRT2_LD) / 2) * B)
        bp[k, 1] = B - bp[k, 0]
    assert ((bp > 0) & (bp < B)).all()
    got = ar.fit(bp, B, rho, 5, precision)
    want = float(LD(1) - ar.erfc_ld(-LD(d - c) / ar.SQRT2_LD) / 2)
    assert got.used.tolist() == [10, 10]
    assert abs(float(got.p_au[0]) - want) < 1e-6
    assert abs(float(got.d[0]) - d) < 1e-5 and abs(float(got.c[0]) - c) < 1e-5
    # the complementary tree lies on the mirrored curve
    assert abs(float(got.d[1]) + d) < 1e-5 and abs(float(got.c[1]) + c) < 1e-5
    assert abs(float(got.p_au[0] + got.p_au[1]) - 1) < 1e-6
    assert float(got.rss[0]) < 1e-4 * 10 and float(got.se[0]) > 0


def test_two_precisions_agree():
    B = 1000
    rho = ar.ratios([ar.draws_of(r, 4385) for r in ar.DEFAULT_SCALES], 4385)
    bp = np.array([[500 + 30 * k, 400 - 25 * k, 100 - 5 * k, 0] for k in range(10)])
    a, b = ar.fit(bp, B, rho, 5, "float64"), ar.fit(bp, B, rho, 5, "longdouble")
    assert a.used.tolist() == b.used.tolist() == [10, 10, 10, 0]
    for name in ("p_au", "d", "c", "se", "rss"):
        assert np.abs(getattr(a, name).astype(LD) - getattr(b, name)).max() < 1e-10
    assert a.p_au.dtype == np.float64 and b.p_au.dtype == LD


def test_fewer_than_two_usable_scales():
    B = 100
    rho = [0.5, 1.0, 1.5]
    #               always   never   once usable   never usable: 0 or B
    bp = np.array([[100,     0,      100,          0],
                   [100,     0,      37,           100],
                   [100,     0,      0,            100]])
    for precision in ("float64", "longdouble"):
        got = ar.fit(bp, B, rho, 1, precision)
        assert got.used.tolist() == [0, 0, 1, 0]
        assert [float(x) for x in got.p_au] == [1.0, 0.0, 0.37, 1.0]
        for name in ("d", "c", "se", "rss"):
            assert not getattr(got, name).any()
        assert [float(x) for x in ar.fit(bp, B, rho, 0, precision).p_au] == [1.0, 0.0, 1.0, 0.0]
    # two usable scales: an exact fit
    bp2 = np.array([[60, 40], [70, 30], [100, 0]])
    got = ar.fit(bp2, B, rho, 1)
    assert got.used.tolist() == [2, 2] and float(got.rss.max()) < 1e-25


# ---------------------------------------------------------------------------
# the shapes of the device tests (tests/au_cases.py)
# ---------------------------------------------------------------------------
def test_shapes_leave_nothing_undecided_and_set_the_fit_tolerance():
    """what the device tests rely on: the reference is certain of every (scale, replicate) row at every shape; the
    constructed shape has trees with used >= 3 and trees with used < 2; FIT_DIFFERENCE is the largest float64 /
    long-double difference of the reference's own fits (from above, within a quarter)"""
    import au_cases as ac
    worst = dict.fromkeys(ac.FIT_DIFFERENCE, 0.0)
    for shape in ac.SHAPES:
        ref = ac.reference_of(shape)
        assert ref.undecided.sum() == 0, ac.shape_id(shape)
        assert (ref.certain == ref.bp_count).all() and (ref.bp_count.sum(axis=1) == shape[2]).all()
        assert len(set(ref.draws)) == shape[3]
        for name, v in ac.fit_differences(shape).items():
            worst[name] = max(worst[name], v)
    print(worst)
    for name, v in worst.items():
        assert ac.FIT_DIFFERENCE[name] / 1.25 <= v <= ac.FIT_DIFFERENCE[name], (name, v)
        assert ac.FIT_TOLERANCE[name] == 16 * ac.FIT_DIFFERENCE[name]
    ref = ac.reference_of(ac.RANKED)
    used = ar.fit(ref.bp_count, ac.RANKED[2], ref.rho, ref.kstar).used
    assert (used >= 3).any() and (used < 2).any()
