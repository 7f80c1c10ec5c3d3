"""Host restatement of the resampling definitions ("Topology tests and bootstrap weights"): the
counter-based draws in uint64 arithmetic, the replicate log-likelihoods and the BP / KH / SH / ELW statistics in
numpy.longdouble.  Test infrastructure: it shares no code with the library."""
import numpy as np

LD = np.longdouble
U64 = np.uint64
MASK32 = U64(0xFFFFFFFF)
GOLDEN = 0x9E3779B97F4A7C15
MAX_DRAWS, MAX_REPLICATES = 1 << 40, 1 << 24


def mix(seed, c):
    """SplitMix64 output for counter(s) c of the stream `seed`: uint64 array"""
    with np.errstate(over="ignore"):
        z = U64(seed & (2**64 - 1)) + (np.asarray(c, dtype=U64) + U64(1)) * U64(GOLDEN)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def mulhi64(u, n):
    """the upper 64 bits of u * n, u a uint64 array and n < 2^40, in 32-bit limbs (no intermediate overflows)"""
    assert 0 <= n < MAX_DRAWS
    u = np.asarray(u, dtype=U64)
    ul, uh, nl, nh = u & MASK32, u >> U64(32), U64(n & 0xFFFFFFFF), U64(n >> 32)
    p0, p1, p2, p3 = ul * nl, uh * nl, ul * nh, uh * nh
    mid = (p0 >> U64(32)) + (p1 & MASK32) + (p2 & MASK32)
    return p3 + (p1 >> U64(32)) + (p2 >> U64(32)) + (mid >> U64(32))


def sites_of(seed, b, n):
    """the n drawn sites of replicate b"""
    assert 0 <= b < MAX_REPLICATES
    c = (U64(b) << U64(40)) | np.arange(n, dtype=U64)
    return mulhi64(mix(seed, c), n)


def counts(weights, seed, first, count):
    """C[count][S] (int64): replicate first + i draws N = sum(w) sites; a site belongs to the pattern s with
    cum[s - 1] <= site < cum[s]"""
    w = np.asarray(weights, dtype=np.int64)
    cum = np.cumsum(w).astype(U64)
    n = int(w.sum())
    out = np.zeros((count, len(w)), dtype=np.int64)
    for i in range(count):
        pattern = np.searchsorted(cum, sites_of(seed, first + i, n), side="right")
        out[i] = np.bincount(pattern, minlength=len(w))
    return out


def counts_brute_force(weights, seed, first, count):
    """the same in plain Python integers"""
    m64 = 2**64 - 1
    w = [int(x) for x in weights]
    n = sum(w)
    out = [[0] * len(w) for _ in range(count)]
    for i in range(count):
        for k in range(n):
            c = ((first + i) << 40) | k
            z = (seed + (c + 1) * GOLDEN) & m64
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
            site = ((z ^ (z >> 31)) * n) >> 64
            s, acc = 0, w[0]
            while site >= acc:
                s += 1
                acc += w[s]
            out[i][s] += 1
    return np.array(out, dtype=np.int64)


def replicates(C, L):
    """R[b][t] = sum_s C[b][s] L[t][s] in long double; with C = w[None, :] the observed log-likelihoods"""
    return np.asarray(C, dtype=LD) @ np.asarray(L, dtype=LD).T


def magnitudes(C, L):
    """sum_s C[b][s] |L[t][s]|: the scale of the rounding-error bound of an fp64 evaluation of replicates()"""
    return np.asarray(C, dtype=LD) @ np.abs(np.asarray(L, dtype=LD)).T


class Stats:
    pass


def margins(R, lnl):
    """The long-double left-hand side minus right-hand side of every decision of the definitions, from replicate
    log-likelihoods R [B][T] and observed lnl [T]:
    bp[b][t] = R[b][t] - max over the other trees (a tree wins replicate b when this is > 0, or == 0 with the lowest
    index), kh[b][t], sh[b][t] >= 0 where the replicate counts."""
    R, lnl = np.asarray(R, dtype=LD), np.asarray(lnl, dtype=LD)
    B, T = R.shape
    best = int(np.argmax(lnl))
    out = Stats()
    out.best = best
    out.bp = np.empty((B, T), dtype=LD)
    for t in range(T):
        others = np.delete(R, t, axis=1)
        out.bp[:, t] = R[:, t] - (others.max(axis=1) if T > 1 else LD(-np.inf))
    delta = lnl[best] - lnl
    d = R[:, [best]] - R
    out.kh = d - d.mean(axis=0) - delta
    Rc = R - R.mean(axis=0)
    out.sh = Rc.max(axis=1)[:, None] - Rc - delta
    e = np.exp(R - R.max(axis=1)[:, None])
    out.elw = (e / e.sum(axis=1)[:, None]).mean(axis=0)
    return out


def statistics(R, lnl):
    """best, bp_count, kh_count, sh_count (int64 [T]) and elw (long double [T]) by the definitions, ties to the lowest
    index"""
    R = np.asarray(R, dtype=LD)
    B, T = R.shape
    m = margins(R, lnl)
    out = Stats()
    out.best, out.elw = m.best, m.elw
    out.bp_count = np.bincount(np.argmax(R, axis=1), minlength=T)
    out.kh_count = (m.kh >= 0).sum(axis=0)
    out.sh_count = (m.sh >= 0).sum(axis=0)
    out.kh_count[m.best] = out.sh_count[m.best] = B        # d == 0 and M_b - R~[b][best] >= 0 exactly
    return out


def decided(R, lnl, tol):
    """per statistic (certain [T], undecided [T]): the replicates whose decision has a margin beyond tol, and those
    within it"""
    m = margins(R, lnl)
    out = Stats()
    out.best, out.elw = m.best, m.elw
    out.bp = ((m.bp > tol).sum(axis=0), (np.abs(m.bp) <= tol).sum(axis=0))
    out.kh = ((m.kh > tol).sum(axis=0), (np.abs(m.kh) <= tol).sum(axis=0))
    out.sh = ((m.sh > tol).sum(axis=0), (np.abs(m.sh) <= tol).sum(axis=0))
    return out
