"""The contract of pllhip_sample_histories_edges ("Sampled substitution histories") restated in numpy
float64 and Python integers, for tests only.  It is fed with what the library under test holds: the tables of its host
stage (pllhip_history_rate_table, pllhip_history_poisson, called with the partition's eigen systems, rates and p-inv
and the caller's lengths), the sampled states and components of the ancestral draw (state indices, tip rows included),
the edge list with its matrix indices, and the pattern weights.  It runs the same operations in the same order, so its
integers are the library's integers: the tests compare with ==, no tolerance and no excluded draws.

    jump count     w_k = pois[m][r][k] Rpow[k][a][c], k < K(m, r)               stream H + (m << 11)
    step i         w_d = R[x_(i-1)][d] Rpow[N - i][d][c], d < S, R = Rpow[1]   stream H + (m << 11) + i
    time i         T_i = mix(key(seed, b, H + (m << 11) + 1024 + i), n) >> 32; event j at the j-th smallest (T, i)
    H = 0x40000000

Every table is cumulated left to right, one add after the other; x = u total is one multiply; the pick is the bisection
(ancsample_reference.cumulate, pick).  A real jump x -> y of a pattern of weight w at time T adds w to counts[x][y],
w T to units[r][x] and -w T to units[r][y]; units[r][c] gains w 2^32 once; everything modulo 2^64.

The uniformization identity (`identity_bound`).  sum_k pois[k] Rpow[k][a][c] is the transition probability
P_r[a][c] = exp(Q tau)[a][c] that the partition holds from its eigen system.  Three things separate the two doubles,
with u = 2^-53, S states, K table entries, lam = mu tau, rho = max |eigenvalue| tau:
    the truncation of the table         2^-70 of the Poisson mass, by the rule that ends it, and the geometric tail behind
                                        it (the ratio lam / k is below 1 there and falling): at most 2 * 2^-70 absolute
    the sum itself                      terms are non-negative, so relative errors do not grow in the sum:
        Rpow[k]                         k matrix products of 2 S - 1 roundings a path, on entries of R that carry the
                                        S + 2 roundings of Q's entry (S products with the eigenvalue, S - 1 additions,
                                        the quotient by mu, mu's own S roundings): k (2 S - 1) + k (3 S + 3)
        pois[k]                         exp, log and lgamma to an ulp each; the roundings of k log lam, of lam and of
                                        lgamma(k + 1) and the two subtractions enter the exponential absolutely, each
                                        at most u times the largest magnitude among the three, M = max(k |log lam|,
                                        lam, lgamma(k + 1)): 2 + 6 M
        product and sum                 1 + K
      together (k <= K)                 k_sum = K (5 S + 2) + 3 + 6 M_max + K
    the partition's own entry           V diag(exp(lambda tau)) V^-1 is a signed sum: its error is relative to the same
                                        expression on absolute values, Pabs = |V| exp(lambda tau) |V^-1| (2 S + 2 + rho
                                        roundings: S products of three factors, S - 1 additions, the exponential and
                                        its argument), not to P itself
    Q as the table sees it              negative off-diagonal entries are clamped to 0 and the diagonal is minus the sum
                                        of the others; for a reversible model both only remove rounding noise of the
                                        size already counted in Rpow
The bound is 2 (k_sum u P + (2 S + 2 + rho) u Pabs) + 2^-69: a factor 2 of margin on the rounding terms."""
import numpy as np

import ancsample_reference as asr
import pllhip_ctypes as pc
import simulate_reference as simr
import sitecat_reference as sr
import substmap_reference as smr

_U = np.uint64
STREAM = 0x40000000
MASK = (1 << 64) - 1


class Tables:
    """slot [R]; mu [slots]; rpow [slots][kmax][S][S]; tau [E][R]; pois: (edge, r) -> [K]"""


def tables(lib, inst, lengths, params_indices=None):
    """the tables of a call, built with the library's own host functions from what the partition holds"""
    p = inst.p.contents
    idx = [int(x) for x in (inst.params if params_indices is None else params_indices)]
    t = Tables()
    distinct = []
    for i in idx:
        if i not in distinct:
            distinct.append(i)
    t.slot = np.array([distinct.index(i) for i in idx])
    eig = [smr.eigen_of(inst, i) for i in distinct]
    t.mu = np.array([pc.history_rate_table(lib, *e, 1, states=inst.S)[0] for e in eig])
    rho = np.array([p.rates[r] for r in range(inst.R)])
    q = np.array([p.prop_invar[i] for i in idx])
    t.tau = np.array([[rho[r] * float(L) / (1.0 - q[r]) for r in range(inst.R)] for L in lengths]).reshape(len(lengths), inst.R)
    t.pois = {(e, r): pc.history_poisson(lib, t.mu[t.slot[r]] * t.tau[e, r]) for e in range(len(lengths)) for r in range(inst.R)}
    t.kmax = max([2] + [len(v) for v in t.pois.values()])
    t.rpow = np.stack([pc.history_rate_table(lib, *e, t.kmax, states=inst.S)[1] for e in eig])
    return t


def time_draw(seed, b, m, i, n):
    return simr.mix(simr.key(seed, b, STREAM + (m << 11) + 1024 + i), n) >> _U(32)


class Result:
    """counts [B][E][S][S], units [B][E][R][S] (uint64, modulo 2^64), changes uint8 [B][E][N], dropped_edges [B][E],
    jumps [B][E][N] (all jumps of the chain, -1 where nothing was drawn), last [B][E][N] (x_N, -1 likewise)"""


def sample(t, states, comp, edges, m, seed, first_replicate=0):
    """states uint8 [B][rows][N] (state indices, tips included), comp uint8 [B][N], edges = (parent, child, matrix) arrays
    in the order of the tables, m [N] pattern weights"""
    B, _, N = states.shape
    parent, child, matrix = (np.asarray(a, dtype=np.int64) for a in edges)
    E, R, S = len(parent), t.tau.shape[1], t.rpow.shape[-1]
    res = Result()
    counts = [[[0] * (S * S) for _ in range(E)] for _ in range(B)]
    units = [[[0] * (R * S) for _ in range(E)] for _ in range(B)]
    res.changes = np.full((B, E, N), 255, dtype=np.uint8)
    res.dropped_edges = np.zeros((B, E), dtype=np.uint64)
    res.jumps = np.full((B, E, N), -1, dtype=np.int64)
    res.last = np.full((B, E, N), -1, dtype=np.int64)
    sites = np.arange(N, dtype=_U)
    w = [int(x) for x in m]
    for i in range(B):
        b = first_replicate + i
        for e in range(E):
            mi = int(matrix[e])
            a_all, c_all = states[i, parent[e]].astype(np.int64), states[i, child[e]].astype(np.int64)
            live = comp[i] != 255
            res.changes[i, e, live & ((comp[i] & 0x80) != 0)] = 0
            for r in range(R):
                sel = np.nonzero(comp[i] == r)[0]
                if not len(sel):
                    continue
                pois, rp = t.pois[(e, r)], t.rpow[t.slot[r]]
                K, R1 = len(pois), t.rpow[t.slot[r]][1]
                a, c, n = a_all[sel], c_all[sel], sites[sel]
                ok = (a < S) & (c < S)
                cum = asr.cumulate(pois[None, :] * rp[:K][:, np.minimum(a, S - 1), np.minimum(c, S - 1)].T)
                total = cum[:, -1]
                ok &= (total > 0) & np.isfinite(total)
                res.dropped_edges[i, e] += int((~ok & (m[sel] > 0)).sum())
                sel, a, c, n, cum = sel[ok], a[ok], c[ok], n[ok], cum[ok]
                if not len(sel):
                    continue
                Nj = asr.pick(simr.uniform(seed, b, STREAM + (mi << 11), n), cum)
                res.jumps[i, e, sel] = Nj
                top = int(Nj.max())
                # the event times in order: (T, i) ascending
                order = np.zeros((len(sel), top), dtype=_U)
                if top:
                    T = np.stack([time_draw(seed, b, mi, s, n) for s in range(1, top + 1)], axis=1)
                    keyed = (T << _U(10)) | np.arange(1, top + 1, dtype=_U)[None, :]
                    keyed = np.where(np.arange(1, top + 1)[None, :] <= Nj[:, None], keyed, _U(MASK))
                    order = np.sort(keyed, axis=1) >> _U(10)
                x, real = a.copy(), np.zeros(len(sel), dtype=np.int64)
                for s in range(1, top + 1):
                    act = np.nonzero(Nj >= s)[0]
                    to = rp[Nj[act] - s, :, c[act]]                        # [site][d]
                    y = asr.pick(simr.uniform(seed, b, STREAM + (mi << 11) + s, n[act]), asr.cumulate(R1[x[act]] * to))
                    for k in np.nonzero(y != x[act])[0]:
                        j, wt = act[k], w[sel[act[k]]]
                        T = int(order[j, s - 1])
                        counts[i][e][int(x[j]) * S + int(y[k])] += wt
                        units[i][e][r * S + int(x[j])] += wt * T
                        units[i][e][r * S + int(y[k])] -= wt * T
                        real[j] += 1
                    x[act] = y
                for j in range(len(sel)):
                    units[i][e][r * S + int(c[j])] += w[sel[j]] << 32
                res.changes[i, e, sel] = np.minimum(real, 254)
                res.last[i, e, sel] = x
    res.counts = np.array([[[v & MASK for v in ce] for ce in cb] for cb in counts], dtype=np.uint64).reshape(B, E, S, S)
    res.units = np.array([[[v & MASK for v in ue] for ue in ub] for ub in units], dtype=np.uint64).reshape(B, E, R, S)
    return res


def summary(tau, counts_int, units):
    """pllhip_history_summary in float64, operation for operation: (counts [S][S], dwell [S], total)"""
    counts = np.asarray(counts_int, dtype=np.uint64).astype(np.float64)
    total = 0.0
    for v in counts.reshape(-1):
        total += v
    signed = np.asarray(units, dtype=np.uint64).view(np.int64).astype(np.float64)
    dwell = np.zeros(signed.shape[1])
    for r in range(signed.shape[0]):
        dwell = dwell + (tau[r] * 2.0 ** -32) * signed[r]
    return counts, dwell, total


def identity_bound(S, pois, lam, eig, tau, P):
    """the bound of the docstring for one (m, r): [S][S]"""
    W, V, ev = eig
    K = len(pois)
    k = np.arange(K)
    from math import lgamma, log
    M = max([abs(kk * log(lam)) for kk in k] + [lam] + [lgamma(kk + 1.0) for kk in k]) if lam > 0 else 0.0
    k_sum = K * (5 * S + 2) + 3 + 6 * M + K
    rho = float(np.max(np.abs(ev)) * tau)
    Pabs = (np.abs(V[:, :S]) * np.exp(ev * tau)[None, :]) @ np.abs(W[:S, :S])
    u = 2.0 ** -53
    return 2.0 * (k_sum * u * np.abs(P) + (2 * S + 2 + rho) * u * Pabs) + 2.0 ** -69
