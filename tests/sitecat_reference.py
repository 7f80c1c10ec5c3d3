"""An exact host reference of the site-category quantities of one edge (include/pllhip.h, "site categories"), for tests
only: everything in numpy.longdouble from what the library under test holds -- its own vectors (a coded tip as the 0/1
expansion of its masks), its own P-matrix, scaler counts, invariant states, frequencies, p-inv, rates and weights.

    l[n][r] = sum_i pi_r[i] parent[n, r, i] sum_j P_r[i][j] child[n, r, j]
    A = (1 - q_r) l,  B = q_r pi_r[invariant[n]],  g = A + B,  T[n] = sum_r w_r g[n][r],  lnl = log T - c 256 ln 2
    post = w_r A / T,  inv = sum_r w_r B / T,  rate = sum_r post rho_r,  expected[r] = sum_n m_n w_r g / T

with the scaling rules of the edge kernels (per-rate counts brought to their minimum by 2^-256 per step, at most four;
a site with an invariant term and c > 0 brought to scale for c <= 3, dropped above, c = 0 then).

Bounds.  The inputs are the engine's doubles and every sum is a sum of non-negative terms, so whatever the order of
summation (the matrix cores included) an fp64 evaluation differs from the exact value by at most k 2^-53 relative, k the
number of roundings on the longest path to the value; 2^-1000 absolute lets products that underflow pass.  Counts, for S
states, R categories and N sites (u = 2^-53):
    table entry     k_tab  = 2 S + 8        S products and S - 1 additions in sum_j, two products and S - 1 additions in
                                            sum_i: 2 S + 2; 1 - q and its product: 2; the rest covers the lookup-table
                                            row of a coded child (its own S - 1 additions, in place of the inner sum)
                                            and the constant factors.  Powers of two (rate factors, descaling) are exact.
    T               k_T    = k_tab + R + 1  A + B, the product with w, R - 1 additions
    posterior       k_post = k_tab + k_T + 2          w A: k_tab + 1; the quotient adds T's own error and one rounding
    invariant part  k_inv  = (R + 2) + k_T + 1
    site rate       k_rate = k_post + R + 1
    expected        k_exp  = k_post + N + 2           g for A, the product with m_n, N - 1 additions
    EM step         k_step = k_exp + R + 1            the divisor sum_r expected[r] and the quotient
Every bound below is 2 k u ref + 2^-1000: a factor 2 of margin.  A table entry below fp64's range is lost absolutely,
not relatively (per-rate scalers bring a category down by up to 2^-1024), and a quotient by T[n] magnifies that loss:
the absolute term of a posterior, an invariant part or a site rate is 2^-1000 (1 + s / T[n]) with s the largest factor on
the entry (1 for a posterior, the largest rate for a site rate), and that of expected[r] the sum of m_n times it.
lnl: T within 2 k_T u relative moves log T by 2 k_T u (1 + 2 k_T u) absolutely; the logarithm, the product c 256 ln 2
(with the constant's own rounding) and the subtraction each round once, the logarithm to an ulp rather than half of
one: 2 u (|log T| + 2 c 256 ln 2 + |lnl|), margin included.  The weighted sum over the sites adds the weighted bounds of
its terms and 2 (N + 1) u sum_n m_n |lnl[n]|."""
import numpy as np

import ancestral_reference as ar
import pllhip_ctypes as pc

LD = np.longdouble
U = LD(2.0) ** -53
TINY = LD(2.0) ** -1000
LN_SCALE = LD(256) * np.log(LD(2))
RATE_MAXDIFF = 4


class Table:
    """A, B [site][cat], c [site] (longdouble, counts as int64), and what they were made under"""


def k_tab(S):
    return 2 * S + 8


def k_T(S, R):
    return k_tab(S) + R + 1


def k_post(S, R):
    return k_tab(S) + k_T(S, R) + 2


def k_inv(S, R):
    return (R + 2) + k_T(S, R) + 1


def k_rate(S, R):
    return k_post(S, R) + R + 1


def k_exp(S, R, N):
    return k_post(S, R) + N + 2


def k_step(S, R, N):
    return k_exp(S, R, N) + R + 1


def bound(ref, k, floor=None):
    """2 k u ref + floor per entry; floor: 2^-1000, or what floor_of gives for a value divided by T"""
    return LD(2 * k) * U * np.asarray(ref, dtype=LD) + (TINY if floor is None else floor)


def floor_of(T, scale=1):
    """the absolute term of a value that is a table entry times `scale` over T[n]: 2^-1000 (1 + scale / T) per site
    (T = 0: 2^-1000, the value is 0)"""
    T = np.asarray(T, dtype=LD)
    return TINY * (1 + np.divide(LD(scale), T, out=np.zeros_like(T), where=T > 0))


def worst(got, ref, k, floor=None):
    """largest |got - ref| as a fraction of the bound (0 for an empty array)"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(got - ref) / bound(ref, k, floor))) if got.size else 0.0


def model_of(inst):
    """what the partition's own arrays say: (pi [cat][state], q [cat], w [cat], rho [cat], m [site], invariant [site])"""
    p = inst.p.contents
    freqs, w = ar.model_of(inst)
    q = np.array([p.prop_invar[int(inst.params[r])] for r in range(inst.R)])
    rho = np.array([p.rates[r] for r in range(inst.R)])
    m = np.array([p.pattern_weights[n] for n in range(inst.N)], dtype=np.int64)
    inv = np.array([p.invariant[n] for n in range(inst.N)], dtype=np.int64) if p.invariant else np.full(inst.N, -1)
    return freqs, q, w, rho, m, inv


def counts_of(inst, scaler):
    """[site][cat] scaler counts of a buffer (the same count for every category without per-rate scalers)"""
    if scaler == pc.PLL_SCALE_BUFFER_NONE:
        return np.zeros((inst.N, inst.R), dtype=np.int64)
    c = inst.get_scaler(scaler).astype(np.int64)
    return c.reshape(inst.N, inst.R) if inst.rate_scalers else np.repeat(c[:, None], inst.R, axis=1)


def table(parent, child, pmatrix, freqs, q, w, counts, invariant):
    """parent / child [site][cat][state], pmatrix [cat][state][state], freqs [cat][state], q / w [cat],
    counts [site][cat] (both ends added), invariant [site] (-1: none)"""
    parent, child, P = np.asarray(parent, dtype=LD), np.asarray(child, dtype=LD), np.asarray(pmatrix, dtype=LD)
    pi, q, w = np.asarray(freqs, dtype=LD), np.asarray(q, dtype=LD), np.asarray(w, dtype=LD)
    N, R, S = parent.shape
    l = np.zeros((N, R), dtype=LD)
    for r in range(R):
        t = np.zeros((N, S), dtype=LD)
        for j in range(S):                                  # t[n][i] = sum_j P_r[i][j] child[n, r, j]
            t += child[:, r, j:j + 1] * P[r, :, j][None, :]
        l[:, r] = (pi[r][None, :] * parent[:, r, :] * t).sum(axis=1)
    c = counts.min(axis=1)
    d = np.minimum(counts - c[:, None], RATE_MAXDIFF)
    l = l * LD(2.0) ** (-256 * d).astype(LD)
    has = invariant >= 0
    v = np.zeros((N, R), dtype=LD)
    for r in range(R):
        if q[r] > 0:
            v[has, r] = pi[r][invariant[has]]
    descale = ((w[None, :] * q[None, :] * v).sum(axis=1) > 0) & (c > 0)
    factor = np.where(c <= 3, LD(2.0) ** (-256 * np.minimum(c, 3)).astype(LD), LD(0))
    l[descale] = l[descale] * factor[descale][:, None]
    out = Table()
    out.A = np.where(q[None, :] > 0, (1 - q)[None, :] * l, l)
    out.B = q[None, :] * v
    out.c = np.where(descale, 0, c)
    return out


def reference(inst, parent, parent_scaler, child, child_scaler, matrix):
    """the table of one edge from what `inst` holds"""
    freqs, q, w, rho, m, inv = model_of(inst)
    counts = counts_of(inst, parent_scaler) + counts_of(inst, child_scaler)
    return table(ar.clv_of(inst, parent), ar.clv_of(inst, child), inst.get_pmatrix(matrix), freqs, q, w, counts, inv)


class Posteriors:
    """T, lnl, post, inv, rate, category, expected, loglh in longdouble"""


def posteriors(A, B, c, w, rho=None, m=None):
    A, B, w = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD), np.asarray(w, dtype=LD)
    N, R = A.shape
    m = np.ones(N, dtype=np.int64) if m is None else np.asarray(m, dtype=np.int64)
    rho = np.zeros(R, dtype=LD) if rho is None else np.asarray(rho, dtype=LD)
    c = np.zeros(N, dtype=np.int64) if c is None else np.asarray(c, dtype=np.int64)
    g = A + B
    out = Posteriors()
    out.T = (w[None, :] * g).sum(axis=1)
    live = out.T > 0
    safe = np.where(live, out.T, LD(1))
    with np.errstate(divide="ignore"):
        out.logT = np.where(live, np.log(safe), -np.inf).astype(LD)
    out.lnl = out.logT - c.astype(LD) * LN_SCALE
    out.post = np.where(live[:, None], w[None, :] * A / safe[:, None], LD(0))
    out.inv = np.where(live, (w[None, :] * B).sum(axis=1) / safe, LD(0))
    out.rate = (out.post * rho[None, :]).sum(axis=1)
    out.category = np.argmax(out.post, axis=1).astype(np.uint8)
    gamma = np.where(live[:, None], w[None, :] * g / safe[:, None], LD(0))
    out.expected = (m[:, None].astype(LD) * gamma).sum(axis=0)
    weighted = m > 0
    out.loglh = (m[weighted].astype(LD) * out.lnl[weighted]).sum() if weighted.any() else LD(0)
    out.c, out.m = c, m
    return out


def em_step(A, B, c, w, m=None):
    """(w' = expected / sum_n m_n, loglh at w)"""
    po = posteriors(A, B, c, w, None, m)
    return po.expected / po.m.astype(LD).sum(), po.loglh


def lnl_bound(po, S, R):
    """per site, for finite lnl (see the module docstring)"""
    rel = LD(2 * k_T(S, R)) * U
    fin = np.isfinite(po.lnl)
    logT, lnl = np.where(fin, po.logT, LD(0)), np.where(fin, po.lnl, LD(0))
    return rel * (1 + rel) + 2 * U * (np.abs(logT) + 2 * po.c.astype(LD) * LN_SCALE + np.abs(lnl))


def loglh_bound(po, S, R):
    w = po.m > 0
    m = po.m[w].astype(LD)
    return (m * lnl_bound(po, S, R)[w]).sum() + LD(2 * (len(po.m) + 1)) * U * (m * np.abs(po.lnl[w])).sum()


def clear_rows(post, S, R):
    """(clear, zero): rows whose two largest reference posteriors differ by more than the bounds of both, and rows that
    are all zero (category 0, probability 0)"""
    if post.shape[1] == 1:
        return np.ones(len(post), dtype=bool), post[:, 0] == 0
    top = np.sort(post, axis=1)
    b = bound(top, k_post(S, R))              # (the largest two of a row: far above the absolute term)
    zero = top[:, -1] == 0
    return (top[:, -1] - top[:, -2] > b[:, -1] + b[:, -2]) & ~zero, zero
