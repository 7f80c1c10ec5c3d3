"""Host restatement of the multiscale bootstrap and the AU test ("Multiscale replicates and the AU
test"): the per-scale streams and draws in uint64 arithmetic, the per-scale decisions in numpy.longdouble, and the
weighted least-squares fit of the (d, c) curve in float64 and in numpy.longdouble.  Test infrastructure: it shares no
code with the library; the generator's primitives come from rell_reference."""
import math

import numpy as np

import rell_reference as rr
from rell_reference import mix, mulhi64, replicates, magnitudes      # noqa: F401  (re-exported for the tests)

LD = np.longdouble
U64 = np.uint64
M64 = 2**64 - 1
MAX_SCALES = 64
DEFAULT_SCALES = tuple(i / 10.0 for i in range(5, 15))


# ---------------------------------------------------------------------------
# scales
# ---------------------------------------------------------------------------
def draws_of(r, N):
    """n_k = floor(r N + 0.5) in double arithmetic; None where the scale itself is refused"""
    if not math.isfinite(r) or r <= 0:
        return None
    return int(math.floor(r * float(N) + 0.5))


def refusal(scales, N, B, trees):
    """the reason the contract gives for refusing a call, or None"""
    if B == 0 or B >= rr.MAX_REPLICATES:
        return "replicates"
    K = 10 if scales is None else len(scales)
    if K < 2 or K > MAX_SCALES:
        return "scales"
    if trees == 0:
        return "empty"
    seen = []
    for r in (DEFAULT_SCALES if scales is None else scales):
        n = draws_of(r, N)
        if n is None:
            return "scale"
        if n < 1 or n >= rr.MAX_DRAWS:
            return "draws"
        if n in seen:
            return "duplicate"
        seen.append(n)
    return None


def nearest_scale(draws, N):
    """k*: the scale whose n_k is nearest to N, lowest k on ties"""
    gaps = [abs(int(n) - int(N)) for n in draws]
    return gaps.index(min(gaps))


# ---------------------------------------------------------------------------
# streams and counts
# ---------------------------------------------------------------------------
def seed_of(seed, k):
    """the stream of scale k: mix(~seed, k)"""
    return int(mix(~seed & M64, k))


def counts(weights, seed, k, n_k, first, count):
    """C_k[count][S] (int64): replicate first + i of scale k draws n_k sites of N = sum(w)"""
    w = np.asarray(weights, dtype=np.int64)
    cum = np.cumsum(w).astype(U64)
    N, S = int(w.sum()), len(w)
    sk = seed_of(seed, k)
    out = np.zeros((count, S), dtype=np.int64)
    step = max(1, (1 << 22) // n_k)                                   # replicates per vectorised block
    for lo in range(0, count, step):
        nb = min(step, count - lo)
        b = np.arange(first + lo, first + lo + nb, dtype=U64)
        assert int(b[-1]) < rr.MAX_REPLICATES
        c = (b[:, None] << U64(40)) | np.arange(n_k, dtype=U64)[None, :]
        pattern = np.searchsorted(cum, mulhi64(mix(sk, c), N), side="right")
        flat = pattern + (np.arange(nb, dtype=np.int64) * S)[:, None]
        out[lo:lo + nb] = np.bincount(flat.ravel(), minlength=nb * S).reshape(nb, S)
    return out


def counts_brute_force(weights, seed, k, n_k, first, count):
    """the same in plain Python integers"""
    w = [int(x) for x in weights]
    N = sum(w)

    def mix_int(s, c):
        z = (s + (c + 1) * rr.GOLDEN) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    sk = mix_int(~seed & M64, k)
    out = [[0] * len(w) for _ in range(count)]
    for i in range(count):
        for j in range(n_k):
            site = (mix_int(sk, ((first + i) << 40) | j) * N) >> 64
            s, acc = 0, w[0]
            while site >= acc:
                s += 1
                acc += w[s]
            out[i][s] += 1
    return np.array(out, dtype=np.int64)


# ---------------------------------------------------------------------------
# proportions
# ---------------------------------------------------------------------------
def margins(R):
    """bp margin [B][T] of one scale's replicate log-likelihoods: R[b][t] - max over the other trees"""
    R = np.asarray(R, dtype=LD)
    B, T = R.shape
    out = np.empty((B, T), dtype=LD)
    for t in range(T):
        others = np.delete(R, t, axis=1)
        out[:, t] = R[:, t] - (others.max(axis=1) if T > 1 else LD(-np.inf))
    return out


def proportions(R):
    """bp_count [T] of one scale by the definition: first maximum"""
    R = np.asarray(R, dtype=LD)
    return np.bincount(np.argmax(R, axis=1), minlength=R.shape[1])


def decided(R, tol):
    """(certain [T], undecided [T]) of one scale: replicates a tree wins by more than tol, and those within tol"""
    m = margins(R)
    return (m > tol).sum(axis=0), (np.abs(m) <= tol).sum(axis=0)


# ---------------------------------------------------------------------------
# the normal distribution in long double
# ---------------------------------------------------------------------------
SQRT2_LD = np.sqrt(LD(2))
SQRTPI_LD = np.sqrt(LD(4) * np.arctan(LD(1)))


def erfc_ld(x):
    """erfc in long double: for 0 <= x < 1 one minus the all-positive series of erf, beyond that the continued
    fraction (modified Lentz); erfc(-x) = 2 - erfc(x)"""
    x = LD(x)
    if x < 0:
        return LD(2) - erfc_ld(-x)
    if x < 1:
        term = x
        total = x
        n = 0
        while term > np.finfo(LD).eps * total * LD(0.01):
            n += 1
            term = term * LD(2) * x * x / LD(2 * n + 1)
            total = total + term
        return LD(1) - LD(2) / SQRTPI_LD * np.exp(-x * x) * total
    # erfc(x) = exp(-x^2) / sqrt(pi) * 1 / (x + (1/2) / (x + 1 / (x + (3/2) / (x + ...))))
    f = x
    c, d = x, LD(0)
    for n in range(1, 100000):
        a = LD(n) / LD(2)
        d = x + a * d
        d = LD(1) / d                                   # (x >= 1 and d >= 0: no zero denominator)
        c = x + a / c
        delta = c * d
        f = f * delta
        if abs(delta - LD(1)) < np.finfo(LD).eps * LD(0.25):
            break
    return np.exp(-x * x) / SQRTPI_LD / f


def upper_tail_inverse_f64(p):
    """z >= 0 with erfc(z / sqrt 2) / 2 = p for 0 < p <= 1/2, float64: bisection, then Newton on math.erfc"""
    lo, hi = 0.0, 40.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(mid / math.sqrt(2.0)) > p:
            lo = mid
        else:
            hi = mid
    z = 0.5 * (lo + hi)
    for _ in range(3):
        z = z + (0.5 * math.erfc(z / math.sqrt(2.0)) - p) / (math.exp(-z * z / 2.0) / math.sqrt(2.0 * math.pi))
    return z


def upper_tail_inverse_ld(p):
    """the same in long double: Newton on erfc_ld from the float64 answer"""
    p = LD(p)
    z = LD(upper_tail_inverse_f64(float(p)))
    for _ in range(4):
        z = z + (erfc_ld(z / SQRT2_LD) / LD(2) - p) / (np.exp(-z * z / LD(2)) / (SQRT2_LD * SQRTPI_LD))
    return z


class Fit:
    pass


def fit(bp_count, B, rho, kstar, precision="longdouble"):
    """The contract's fit for every tree from bp_count [K][T], B and the realised ratios rho [K].  z of a usable scale
    comes from the smaller tail: -Phi^-1(p) = sqrt 2 erfcinv(2 p) = -sqrt 2 erfcinv(2 (1 - p)).  Returns a Fit with
    p_au, d, c, se, rss (arrays of the chosen precision) and used (int64)."""
    ld = precision == "longdouble"
    F = LD if ld else np.float64
    inverse = upper_tail_inverse_ld if ld else upper_tail_inverse_f64
    erfc = erfc_ld if ld else math.erfc
    sqrt2 = SQRT2_LD if ld else F(math.sqrt(2.0))
    sqrt2pi = SQRT2_LD * SQRTPI_LD if ld else F(math.sqrt(2.0 * math.pi))
    bp = np.asarray(bp_count, dtype=np.int64)
    K, T = bp.shape
    out = Fit()
    out.used = np.zeros(T, dtype=np.int64)
    for name in ("p_au", "d", "c", "se", "rss"):
        setattr(out, name, np.zeros(T, dtype=F))
    for t in range(T):
        rows = []
        for k in range(K):
            n = int(bp[k, t])
            if not 0 < n < B:
                continue
            p, q = F(n) / F(B), F(B - n) / F(B)
            z = F(inverse(p)) if 2 * n <= B else -F(inverse(q))
            phi = np.exp(-(z * z) / F(2)) / sqrt2pi
            x1 = np.sqrt(F(rho[k]))
            rows.append((z, F(B) * (phi * phi) / (p * q), x1, F(1) / x1))
        out.used[t] = len(rows)
        if len(rows) < 2:
            out.p_au[t] = F(int(bp[kstar, t])) / F(B)
            continue
        a11 = a12 = a22 = b1 = b2 = F(0)
        for z, w, x1, x2 in rows:
            a11 += w * (x1 * x1)
            a12 += w * (x1 * x2)
            a22 += w * (x2 * x2)
            b1 += w * (x1 * z)
            b2 += w * (x2 * z)
        det = a11 * a22 - a12 * a12
        d, c = (a22 * b1 - a12 * b2) / det, (a11 * b2 - a12 * b1) / det
        rss = F(0)
        for z, w, x1, x2 in rows:
            e = z - (d * x1 + c * x2)
            rss += w * (e * e)
        x = d - c
        out.p_au[t] = F(1) - F(erfc(-x / sqrt2)) / F(2)
        out.d[t], out.c[t], out.rss[t] = d, c, rss
        out.se[t] = np.exp(-(x * x) / F(2)) / sqrt2pi * np.sqrt((a11 + a22 + F(2) * a12) / det)
    return out


def ratios(draws, N):
    """rho_k = n_k / N, one double division each (what the library fits with)"""
    return [float(int(n)) / float(int(N)) for n in draws]
