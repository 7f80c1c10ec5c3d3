"""Pairwise state-pair counts and distances, restated in numpy ("Pairwise distances and neighbour
joining"): what pllhip_distances_partition / pllhip_distances_msa must return.

Counts are exact integers.  The p and JC distances are the same double operations the device makes.  The ML distance
is the root of lnL'(t) found by bisection in numpy.longdouble; lnL' needs dP/dt, which no pll call returns, so P(t) and
its derivative are made here from the eigen-decomposition the oracle's pll_update_eigen leaves in the partition
(P = inv_eigenvecs exp(eigenvals rate t / (1 - pinv)) eigenvecs), and tests/test_distance_reference.py holds that P
against the oracle's pll_update_prob_matrices."""
import numpy as np

NONE = 0xFF
LD = np.longdouble


def codes_of_masks(masks, S):
    """state masks (Python ints / uint64, [T][L]) -> uint8 codes: the state of a one-bit mask, NONE otherwise"""
    masks = np.asarray(masks, dtype=np.uint64) & np.uint64((1 << S) - 1)
    out = np.full(masks.shape, NONE, dtype=np.uint8)
    for k in range(S):
        out[masks == np.uint64(1 << k)] = k
    return out


def codes_of_rows(rows, cmap, S):
    """raw characters [T][L] (uint8) and a 256-entry character -> mask map"""
    table = np.array([int(x) for x in cmap], dtype=np.uint64)
    return codes_of_masks(table[np.asarray(rows, dtype=np.uint8)], S)


def counts(codes, weights, S):
    """N[T][T][S][S] int64: N[i][j][a][b] = sum over sites of w [code_i = a] [code_j = b]"""
    T, L = codes.shape
    w = np.ones(L, dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    assert int(w.sum()) < 2 ** 53                         # the float64 product below is exact
    X = (codes[:, None, :] == np.arange(S, dtype=np.uint8)[None, :, None]).astype(np.float64).reshape(T * S, L)
    N = np.rint((X * w[None, :]) @ X.T).astype(np.int64)
    return N.reshape(T, S, T, S).transpose(0, 2, 1, 3).copy()


def compared(codes, weights):
    """n[T][T]: weight of the sites where both taxa have a state, counted without the table"""
    w = np.ones(codes.shape[1], dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    have = (codes != NONE).astype(np.int64)
    return (have * w[None, :]) @ have.T


def p_matrix(N, max_dist=10.0):
    """(n - tr N) / n, one division; max_dist where n = 0; zero diagonal"""
    n = N.sum(axis=(2, 3))
    tr = np.trace(N, axis1=2, axis2=3)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (n - tr).astype(np.float64) / n.astype(np.float64)
    d[n == 0] = max_dist
    np.fill_diagonal(d, 0.0)
    return d


def jc_matrix(N, S, max_dist=10.0):
    """-b log(1 - p / b), b = (S - 1) / S; max_dist where p >= b or n = 0"""
    n = N.sum(axis=(2, 3))
    p = p_matrix(N, 0.0)
    b = np.float64(S - 1) / np.float64(S)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = -b * np.log(1.0 - p / b)
    d[p >= b] = max_dist
    d[n == 0] = max_dist
    np.fill_diagonal(d, 0.0)
    return d


class Model:
    """the eigen-decomposition, rates and p-inv of parameter set 0 of a partition (a pllhip_ctypes.Instance of the
    oracle after pll_update_eigen), in numpy.longdouble"""

    def __init__(self, inst):
        p = inst.p.contents
        S, Sp, R = p.states, p.states_padded, p.rate_cats
        if not p.eigen_decomp_valid[0]:
            assert inst.L.pll_update_eigen(inst.p, 0)
        grab = lambda ptr, n: np.ctypeslib.as_array(ptr, shape=(n,)).copy()
        self.S, self.R = S, R
        self.V = grab(p.inv_eigenvecs[0], S * Sp).reshape(S, Sp)[:, :S].astype(LD)
        self.Vi = grab(p.eigenvecs[0], S * Sp).reshape(S, Sp)[:S, :S].astype(LD)
        self.evals = grab(p.eigenvals[0], Sp)[:S].astype(LD)
        self.rates = grab(p.rates, R).astype(LD)
        self.rate_w = grab(p.rate_weights, R).astype(LD)
        self.pinv = LD(p.prop_invar[0])

    def pmatrix(self, t, r):
        """P^r(t) [S][S]"""
        e = np.exp(self.evals * (self.rates[r] * LD(t) / (LD(1) - self.pinv)))
        return (self.V * e[None, :]) @ self.Vi

    def mixture(self, t):
        """f, f', f'' [S][S]: (1 - pinv) sum_r w_r P^r(t) + pinv I and its derivatives in t"""
        t = LD(t)
        g = np.zeros((3, self.S), dtype=LD)
        for r in range(self.R):
            c = self.evals * (self.rates[r] / (LD(1) - self.pinv))
            e = self.rate_w[r] * np.exp(c * t)
            g[0] += e
            g[1] += c * e
            g[2] += c * c * e
        q = LD(1) - self.pinv
        f = [q * ((self.V * g[k][None, :]) @ self.Vi) for k in range(3)]
        f[0] = f[0] + self.pinv * np.eye(self.S, dtype=LD)
        return f

    def dlnl(self, Nij, t):
        """lnL'(t) of one pair's counts"""
        f, f1, _ = self.mixture(t)
        nz = Nij != 0
        return np.sum(Nij[nz].astype(LD) * (f1[nz] / f[nz]))


def ml_distance(model, Nij, min_dist=1e-6, max_dist=10.0):
    """the maximiser of lnL over [min_dist, max_dist]: min_dist where lnL'(min_dist) <= 0, max_dist where
    lnL'(max_dist) >= 0, else the root of lnL' by bisection (longdouble), rounded to double"""
    if Nij.sum() == 0:
        return max_dist
    lo, hi = LD(min_dist), LD(max_dist)
    if model.dlnl(Nij, lo) <= 0:
        return float(min_dist)
    if model.dlnl(Nij, hi) >= 0:
        return float(max_dist)
    for _ in range(200):
        mid = (lo + hi) / 2
        if mid == lo or mid == hi:
            break
        if model.dlnl(Nij, mid) > 0:
            lo = mid
        else:
            hi = mid
    return float((lo + hi) / 2)


def ml_matrix(model, N, min_dist=1e-6, max_dist=10.0):
    T = N.shape[0]
    d = np.zeros((T, T))
    for i in range(T):
        for j in range(i + 1, T):
            d[i, j] = d[j, i] = ml_distance(model, N[i, j], min_dist, max_dist)
    return d
