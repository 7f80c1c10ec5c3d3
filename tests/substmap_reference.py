"""An exact host reference of the substitution map of one edge (include/pllhip.h, "substitution mapping"), for tests
only: numpy.longdouble from what the library under test holds -- its vectors (a coded tip as the 0/1 expansion of its
masks), its P-matrix, scaler counts, invariant states, frequencies, p-inv, rates, weights and eigen system.

    s[n][r] = w_r (1 - q_r) d[n][r] / T[n]              (0 where T[n] = 0; A, T: tests/sitecat_reference.py)
    J[n][r][i][j] = s pi_r[i] parent[n,r,i] P_r[i][j] child[n,r,j]
    F[r][i][j] = sum_n m_n s pi_r[i] parent[n,r,i] child[n,r,j],  pairs = F o P,  posterior[r] = sum_ij pairs[r]
    differ[n] = sum_r sum_(i != j) J[n][r][i][j]
    K[k][l] = tau e^(lambda_l tau) phi((lambda_k - lambda_l) tau),  G = V^T F V^-T,  M = V^-T (G o K) V^T
    counts[a][b] = q_ab M[a][b] (a != b),  dwell[a] = M[a][a]

Bounds of the device stage.  The inputs are the engine's doubles and every sum is a sum of non-negative terms, so an
fp64 evaluation in ANY order of summation (the matrix cores included) is off by at most k u relative, u = 2^-53, k the
number of roundings on the longest path.  With k_tab(S) and k_T(S, R) of tests/sitecat_reference.py:
    scale m s       k_T + 5         1 - q and its product with d (a power of two): 2; the product with w: 1; the
                                    quotient by T: T's own k_T and 1; the product with m_n: 1
    F               k_F = k_T + N + 7       (scale parent) child: 2; N - 1 additions in any order, workgroup partials
                                    and their sum included (N terms in all); the product with pi: 1
    pairs           k_F + 1         the product with P
    posterior       k_F + S^2       S^2 - 1 additions
    differ          k_tab + k_T + R + 1     the table entry under the zeroed diagonal: k_tab; w: 1; the quotient: k_T + 1;
                                    R - 1 additions
Every bound is 2 k u ref + floor (a factor 2 of margin, as in sitecat_reference).  The floor is that of a value divided
by T there: 2^-1000 (1 + 1 / T[n]) per site (vector entries are at most 1), summed with the pattern weights for F.

Bounds of the host stage.  Its sums are signed, so the error is relative to the same expressions on absolute values:
    Gabs = |V|^T |F| |V^-1|^T,  Mabs = |V^-1|^T (Gabs o K) |V|^T,  qabs = |V| |Lambda| |V^-1|
Four matrix products of length S follow one another (S roundings each along a path: S products, S - 1 additions), the
product with K adds one, and K itself carries k_K = 8 + 3 max|lambda| tau: exp and expm1 to an ulp (2 u each), the
products lambda tau and (lambda_k - lambda_l) tau, whose rounding the exponential magnifies by its argument (at most
max|lambda| tau each, the difference included), the quotient and two products.  q_ab adds S + 2 on qabs.  So
    gamma(S) = 4 S + k_K + S + 4,   |dwell - ref| <= 2 gamma u Mabs[a][a],   |counts - ref| <= 2 gamma u qabs Mabs
and an F that is itself off by dF moves the results by at most the same absolute expressions evaluated at dF."""
import numpy as np

import ancestral_reference as ar
import sitecat_reference as sr

LD = sr.LD
U = sr.U
TINY = sr.TINY


def k_F(S, R, N):
    return sr.k_T(S, R) + N + 7


def k_pairs(S, R, N):
    return k_F(S, R, N) + 1


def k_posterior(S, R, N):
    return k_F(S, R, N) + S * S


def k_differ(S, R):
    return sr.k_tab(S) + sr.k_T(S, R) + R + 1


def descaling(counts, pi, q, w, inv):
    """(1 - q_r) d[n][r] [site][cat]: what the table does to l = 1 (the rules of sitecat_reference.table);
    counts [site][cat]: the scaler counts of both ends added"""
    N, R = counts.shape
    c = counts.min(axis=1)
    d = LD(2.0) ** (-256 * np.minimum(counts - c[:, None], sr.RATE_MAXDIFF)).astype(LD)
    has = inv >= 0
    v = np.zeros((N, R), dtype=LD)
    for r in range(R):
        if q[r] > 0:
            v[has, r] = pi[r][inv[has]]
    descale = ((w[None, :] * q[None, :] * v).sum(axis=1) > 0) & (c > 0)
    factor = np.where(c <= 3, LD(2.0) ** (-256 * np.minimum(c, 3)).astype(LD), LD(0))
    d[descale] = d[descale] * factor[descale][:, None]
    return np.where(q[None, :] > 0, (1 - q)[None, :] * d, d)


class Edge:
    """tab, T, s [site][cat], F / pairs [cat][S][S], posterior [cat], differ [site], dropped, floor_site [site], floor_F"""


def tables(parent, child, pmatrix, freqs, q, w, counts, inv, m):
    """parent / child [site][cat][state], pmatrix [cat][state][state], freqs [cat][state], q / w [cat], counts [site][cat]
    (both ends added), inv [site] (-1: none), m [site]"""
    pi, q, w = np.asarray(freqs, dtype=LD), np.asarray(q, dtype=LD), np.asarray(w, dtype=LD)
    m, inv, counts = np.asarray(m, dtype=np.int64), np.asarray(inv, dtype=np.int64), np.asarray(counts, dtype=np.int64)
    out = Edge()
    out.tab = sr.table(parent, child, pmatrix, pi, q, w, counts, inv)
    out.parent, out.child, out.P = np.asarray(parent, dtype=LD), np.asarray(child, dtype=LD), np.asarray(pmatrix, dtype=LD)
    out.pi, out.m = pi, m
    out.T = (w[None, :] * (out.tab.A + out.tab.B)).sum(axis=1)
    live = out.T > 0
    safe = np.where(live, out.T, LD(1))
    D = descaling(counts, pi, q, w, inv)
    out.s = np.where(live[:, None], w[None, :] * D / safe[:, None], LD(0))
    N, R, S = out.parent.shape
    out.F = np.zeros((R, S, S), dtype=LD)
    out.differ = np.zeros(N, dtype=LD)
    P0 = out.P.copy()
    for r in range(R):
        np.fill_diagonal(P0[r], LD(0))
        left = (m.astype(LD) * out.s[:, r])[:, None] * pi[r][None, :] * out.parent[:, r, :]
        out.F[r] = left.T @ out.child[:, r, :]
        t0 = out.child[:, r, :] @ P0[r].T                      # t0[n][i] = sum_(j != i) P[i][j] child[n][j]
        out.differ += out.s[:, r] * (pi[r][None, :] * out.parent[:, r, :] * t0).sum(axis=1)
    out.pairs = out.F * out.P
    out.posterior = out.pairs.sum(axis=(1, 2))
    out.dropped = int(((m > 0) & ~live).sum())
    out.floor_site = sr.floor_of(out.T)
    out.floor_F = (m.astype(LD) * out.floor_site).sum() + TINY
    return out


def reference(inst, parent, parent_scaler, child, child_scaler, matrix):
    """the tables of one edge from what `inst` holds"""
    freqs, q, w, rho, m, inv = sr.model_of(inst)
    counts = sr.counts_of(inst, parent_scaler) + sr.counts_of(inst, child_scaler)
    return tables(ar.clv_of(inst, parent), ar.clv_of(inst, child), inst.get_pmatrix(matrix), freqs, q, w, counts, inv, m)


def joint(ref, n, r):
    """J[n][r] [S][S]"""
    return ref.s[n, r] * (ref.pi[r] * ref.parent[n, r])[:, None] * ref.P[r] * ref.child[n, r][None, :]


def bound(ref, k, floor):
    return LD(2 * k) * U * np.abs(np.asarray(ref, dtype=LD)) + floor


def worst(got, ref, k, floor):
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(got - ref) / bound(ref, k, floor))) if got.size else 0.0


# ---------------------------------------------------------------------------
# the host stage
# ---------------------------------------------------------------------------
def eigen_of(inst, index=0):
    """(eigenvecs [S][Sp], inv_eigenvecs [S][Sp], eigenvals [S]) of a rate matrix as the partition holds them"""
    p = inst.p.contents
    S, Sp = inst.S, inst.Sp
    ev = np.ctypeslib.as_array(p.eigenvecs[index], shape=(S * Sp,)).copy().reshape(S, Sp)
    iv = np.ctypeslib.as_array(p.inv_eigenvecs[index], shape=(S * Sp,)).copy().reshape(S, Sp)
    lam = np.ctypeslib.as_array(p.eigenvals[index], shape=(Sp,)).copy()[:S]
    return ev, iv, lam


def phi(x):
    x = np.asarray(x, dtype=LD)
    safe = np.where(x == 0, LD(1), x)
    return np.where(x == 0, LD(1), np.expm1(safe) / safe)


def kernel(lam, tau):
    """K[k][l], symmetric"""
    lam, tau = np.asarray(lam, dtype=LD), LD(tau)
    return tau * np.exp(lam[None, :] * tau) * phi((lam[:, None] - lam[None, :]) * tau)


def counts(eigenvecs, inv_eigenvecs, eigenvals, tau, F, absolute=False):
    """(counts [S][S], dwell [S]) in longdouble; absolute: the same expressions on |V|, |V^-1|, |F|, |lambda|"""
    S = len(F)
    W, V, lam = (np.asarray(x, dtype=LD) for x in (eigenvecs, inv_eigenvecs, eigenvals))
    W, V, F = W[:, :S], V[:, :S], np.asarray(F, dtype=LD)
    K = kernel(lam, tau)
    if absolute:
        W, V, F = np.abs(W), np.abs(V), np.abs(F)
    G = V.T @ F @ W.T
    M = W.T @ (G * K) @ V.T
    q = V @ np.diag(np.abs(lam) if absolute else lam) @ W
    c = q * M
    np.fill_diagonal(c, LD(0))
    return c, np.diag(M).copy()


def gamma(S, lam, tau):
    return 4 * S + 8 + 3 * float(np.max(np.abs(lam)) * tau) + S + 4


def counts_bound(eigenvecs, inv_eigenvecs, eigenvals, tau, F, dF=None):
    """(bound of counts, bound of dwell): 2 gamma u on the absolute expressions, plus those at dF"""
    S = len(F)
    g = LD(2 * gamma(S, np.asarray(eigenvals)[:S], tau)) * U
    ca, da = counts(eigenvecs, inv_eigenvecs, eigenvals, tau, F, absolute=True)
    bc, bd = g * ca + TINY, g * da + TINY
    if dF is not None:
        ca, da = counts(eigenvecs, inv_eigenvecs, eigenvals, tau, dF, absolute=True)
        bc, bd = bc + ca, bd + da
    return bc, bd


def taus(inst, length):
    """tau_r = rates[r] t / (1 - q_r)"""
    _, q, w, rho, m, inv = sr.model_of(inst)
    return np.asarray(rho, dtype=LD) * LD(length) / (1 - np.asarray(q, dtype=LD))


def branch(inst, ref, length, dF=None):
    """(counts, dwell, bound of counts, bound of dwell) of an edge summed over the categories, from the reference's F"""
    S, R = inst.S, inst.R
    c, d = np.zeros((S, S), dtype=LD), np.zeros(S, dtype=LD)
    bc, bd = np.zeros((S, S), dtype=LD), np.zeros(S, dtype=LD)
    for r, tau in enumerate(taus(inst, length)):
        eig = eigen_of(inst, int(inst.params[r]))
        cr, dr = counts(*eig, tau, ref.F[r])
        br = counts_bound(*eig, tau, ref.F[r], None if dF is None else dF[r])
        c, d, bc, bd = c + cr, d + dr, bc + br[0], bd + br[1]
    # (the sum over the categories: R - 1 more roundings on values the terms' bounds already cover)
    return c, d, bc * (1 + LD(2 * R) * U), bd * (1 + LD(2 * R) * U)


def derivative(inst, ref, length):
    """(sum_r sum_ij F_r o dP_r/dt, its conditioning: the same sum with every term taken absolutely, in state space and in
    the eigen basis the sumtable of pll_compute_likelihood_derivatives lives in)"""
    _, q, w, rho, m, inv = sr.model_of(inst)
    total, cond = LD(0), LD(0)
    for r, tau in enumerate(taus(inst, length)):
        W, V, lam = (np.asarray(x, dtype=LD) for x in eigen_of(inst, int(inst.params[r])))
        S = inst.S
        W, V = W[:, :S], V[:, :S]
        speed = LD(rho[r]) / (1 - LD(q[r]))
        diag = lam * speed * np.exp(lam * tau)
        dP = V @ np.diag(diag) @ W
        total += (ref.F[r] * dP).sum()
        left = ((ref.m.astype(LD) * ref.s[:, r])[:, None] * ref.pi[r][None, :] * ref.parent[:, r, :]) @ np.abs(V)   # [n][k]
        right = ref.child[:, r, :] @ np.abs(W).T                                                                  # [n][k]
        cond += (left * right * np.abs(diag)[None, :]).sum() + np.abs(ref.F[r] * dP).sum()
    return total, cond
