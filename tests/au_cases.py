"""The shapes, inputs and host references the AU tests share (tests/test_au_gpu.py on the device,
tests/test_au_reference.py for what can be checked without one).  A shape is (S, T, B, K, weights, rows)."""
import functools

import numpy as np

import au_reference as ar
import rell_reference as rr

LD = np.longdouble
SEED = 0x5EED0000BEEF
CHUNK = 1024            # patterns per partial sum up to 65536 patterns
HEAVY = 4000            # the heavy pattern of the mixed weights (70000 in the counts test, where few rows are drawn)

S_SWEEP = [1, 5, 63, 65, 257, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5]
SHAPES = ([(S, 5, 100, 10, "mixed", "noisy") for S in S_SWEEP] +
          [(S, 5, 100, 10, "unit", "noisy") for S in (65, 257, CHUNK + 1)] +
          [(257, T, 100, 10, "mixed", "noisy") for T in (1, 2, 16, 17, 33)] +
          [(257, 5, B, 10, "mixed", "noisy") for B in (1, 15, 17, 1000)] +
          [(257, 5, 48, K, "mixed", "noisy") for K in (2, 3, 64)] +
          [(257, 4, 100, 10, "mixed", "ranked")])
RANKED = SHAPES[-1]      # one row clearly best, two rows close to it, one far worse: used >= 3 and used < 2 together


def shape_id(shape):
    return "S%d-T%d-B%d-K%d-%s-%s" % shape


def scales_of(K):
    """None = the library's ten; otherwise K values from 0.5 to 1.4"""
    return None if K == 10 else np.linspace(0.5, 1.4, K)


@functools.lru_cache(maxsize=None)
def weights_of(S, kind, heavy=HEAVY):
    """unit: all 1; mixed: weights 0 .. 3, zeros included, one heavy pattern"""
    if kind == "unit":
        w = np.ones(S, np.uint32)
    else:
        rng = np.random.default_rng(1000 + S)
        w = rng.integers(0, 4, S).astype(np.uint32)
        if S > 3:
            w[1] = 0
        w[S // 2] = heavy
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def rows_of(S, T, kind, rows):
    """noisy: L[t][s] = base_s + noise, base_s = -Gamma(2, 4), sigma 0.3 (1e-4 at the heavy pattern), one value -1e4.
    ranked (T = 4): row 0 = base; rows 1, 2 = base + noise, shifted so that lnl_t - lnl_0 is -1.0 and -1.3 standard
    deviations of the resampled difference; row 3 = base - 5."""
    rng = np.random.default_rng(2000 + 7 * S + T)
    base = -rng.gamma(2.0, 4.0, S)
    sigma = np.full(S, 0.3)
    sigma[S // 2] = 1e-4
    noise = sigma[None, :] * rng.standard_normal((T, S))
    if rows == "noisy":
        L = base[None, :] + noise
        L[T - 1, S - 1] = -1e4
    else:
        assert T == 4
        w = weights_of(S, kind).astype(np.float64)
        L = np.repeat(base[None, :], T, axis=0)
        for t, m in ((1, 1.0), (2, 1.3)):
            sd = np.sqrt((w * noise[t] ** 2).sum())
            L[t] += noise[t] - ((w * noise[t]).sum() + m * sd) / w.sum()
        L[3] -= 5.0
    L.setflags(write=False)
    return L


class Reference:
    """of one shape: scales (or None), draws n_k [K], rho [K], kstar, C [K] of [B][S], R [K][B][T] (long double),
    bound [K][B][T] (the contract's bound of R), lnl / bound_lnl [T], bp_count [K][T] by the definition,
    certain / undecided [K][T] at 4 x the largest bound"""


@functools.lru_cache(maxsize=None)
def reference_of(shape):
    S, T, B, K, kind, rows = shape
    w, L = weights_of(S, kind), rows_of(S, T, kind, rows)
    N = int(w.astype(np.int64).sum())
    ref = Reference()
    ref.N, ref.scales = N, scales_of(K)
    ref.draws = [ar.draws_of(r, N) for r in (ar.DEFAULT_SCALES if ref.scales is None else ref.scales)]
    assert ar.refusal(ref.scales, N, B, T) is None
    ref.rho, ref.kstar = ar.ratios(ref.draws, N), ar.nearest_scale(ref.draws, N)
    unit = LD(2 * (S + 4)) * LD(2) ** -53
    ref.C = [ar.counts(w, SEED, k, ref.draws[k], 0, B) for k in range(K)]
    ref.R = np.stack([rr.replicates(C, L) for C in ref.C])
    ref.bound = np.stack([unit * rr.magnitudes(C, L) for C in ref.C])
    ref.lnl = rr.replicates(w[None, :], L)[0]
    ref.bound_lnl = unit * rr.magnitudes(w[None, :], L)[0]
    ref.tol = 4 * ref.bound.max()
    ref.bp_count = np.stack([ar.proportions(ref.R[k]) for k in range(K)])
    decisions = [ar.decided(ref.R[k], ref.tol) for k in range(K)]
    ref.certain = np.stack([c for c, _ in decisions])
    ref.undecided = np.stack([u for _, u in decisions])
    return ref


# The tolerance of the fit (rule: 16 x the largest difference between the reference's float64 and long-double fits of
# its own bp_count over SHAPES, per quantity; test_au_reference.py recomputes the differences and checks the rule).
# Measured differences: p_au 1.357e-13, d 1.788e-13, c 1.621e-13, se 2.137e-13, rss 2.628e-14 (the largest come from
# trees with two usable scales, where the 2 x 2 system is the least well conditioned), so the tolerances are
# p_au 2.2e-12, d 2.9e-12, c 2.6e-12, se 3.5e-12, rss 4.3e-13.
FIT_DIFFERENCE = {"p_au": 1.36e-13, "d": 1.79e-13, "c": 1.63e-13, "se": 2.14e-13, "rss": 2.63e-14}
FIT_TOLERANCE = {name: 16 * v for name, v in FIT_DIFFERENCE.items()}


def fit_differences(shape):
    """|float64 fit - long-double fit| of the reference's bp_count of a shape: {quantity: largest over the trees}"""
    S, T, B, K, _, _ = shape
    ref = reference_of(shape)
    a, b = (ar.fit(ref.bp_count, B, ref.rho, ref.kstar, p) for p in ("float64", "longdouble"))
    assert a.used.tolist() == b.used.tolist()
    return {name: float(np.abs(getattr(a, name).astype(LD) - getattr(b, name)).max()) for name in FIT_DIFFERENCE}
