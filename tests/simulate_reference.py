"""The generative process of pllhip_simulate_edges ("Simulated alignments") restated in numpy,
vectorised over sites, with the transition matrices as an argument.

key(b, k) = mix(seed, (b << 32) | k); u(b, k, j) = (mix(key(b, k), j) >> 11) * 2^-53; streams k: 0 the category,
1 invariance, 2 the root state, 3 + matrix index the edge that uses that matrix.  Tables are cumulated left to
right in fp64 with entries below 0 counted as 0; pick(u, cum) = #{s in 0 .. n-2 : cum[s] <= u}."""
import numpy as np

_U = np.uint64


def mix(seed, c):
    """SplitMix64 output number c + 1 of the stream `seed` (rell_mix); seed and c broadcast"""
    with np.errstate(over="ignore"):
        z = np.asarray(seed, dtype=_U) + (np.asarray(c, dtype=_U) + _U(1)) * _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def key(seed, b, k):
    return mix(_U(seed), (_U(b) << _U(32)) | _U(k))


def uniform(seed, b, k, j):
    """u(b, k, j) for an array of absolute site numbers j"""
    return (mix(key(seed, b, k), j) >> _U(11)).astype(np.float64) * 2.0 ** -53


def cumulate(x):
    """running sums along the last axis, one add after the other, entries below 0 (and NaN) as 0"""
    x = np.asarray(x, dtype=np.float64)
    x = np.where(x > 0.0, x, 0.0)
    out = np.empty_like(x)
    acc = np.zeros(x.shape[:-1])
    for s in range(x.shape[-1]):
        acc = acc + x[..., s]
        out[..., s] = acc
    return out


def pick(u, cum):
    """the counting definition: u [...], cum [..., n] -> the number of s in 0 .. n-2 with cum[s] <= u"""
    return (cum[..., :-1] <= np.asarray(u)[..., None]).sum(axis=-1)


def pick_bisect(u, cum):
    """the same number by the bisection the kernel runs (one row: cum [n], scalar u)"""
    lo, hi = 0, len(cum) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if cum[mid] > u:
            hi = mid
        else:
            lo = mid + 1
    return lo


def simulate(seed, sites, replicates, weights, pinv, freqs, pmats, root, edges, tips, node_count, inner=False,
             first_site=0, first_replicate=0):
    """weights [R]; pinv [R] and freqs [R][S] already taken through params_indices; pmats: matrix index -> [R][S][S];
    edges: (parent, child, matrix) triples in any order.  uint8 [replicates][rows][sites], row = node index, rows =
    tips, or node_count with `inner` (rows of nodes the edges do not name: 255)."""
    cumw = cumulate(weights)
    cumf = cumulate(freqs)
    pinv = np.asarray(pinv, dtype=np.float64)
    cump = {m: cumulate(pmats[m]) for m in {e[2] for e in edges}}
    kids = {}
    for p, c, m in edges:
        kids.setdefault(int(p), []).append((int(c), int(m)))
    rows = node_count if inner else tips
    out = np.full((replicates, rows, sites), 255, dtype=np.uint8)
    j = np.arange(sites, dtype=_U) + _U(first_site)
    for r in range(replicates):
        b = first_replicate + r
        cat = pick(uniform(seed, b, 0, j), cumw[None, :])
        invariant = uniform(seed, b, 1, j) < pinv[cat]
        state = {root: pick(uniform(seed, b, 2, j), cumf[cat])}
        order = [root]
        for node in order:
            for child, m in kids.get(node, ()):
                drawn = pick(uniform(seed, b, 3 + m, j), cump[m][cat, state[node]])
                state[child] = np.where(invariant, state[node], drawn)
                order.append(child)
        for node, s in state.items():
            if node < rows:
                out[r, node] = s.astype(np.uint8)
    return out


def model_arrays(inst):
    """(weights [R], pinv [R], freqs [R][S]) of an Instance's host model arrays, through its params_indices"""
    p = inst.p.contents
    R, S = inst.R, inst.S
    idx = [int(x) for x in inst.params]
    weights = np.array([p.rate_weights[c] for c in range(R)])
    pinv = np.array([p.prop_invar[i] for i in idx])
    freqs = np.array([[p.frequencies[i][s] for s in range(S)] for i in idx])
    return weights, pinv, freqs


def accept(counts, expected):
    """the acceptance condition of the statistical tests: with n draws in all, every cell with expectation n p >= 100
    has |count - n p| <= 6 sqrt(n p (1 - p)); the other cells are pooled into one, which is held to the condition
    when its pooled expectation reaches 100 (below that the normal bound says nothing about a count).
    Returns the list of violations (empty: accepted) as (cell, count, expectation, bound)."""
    counts = np.asarray(counts, dtype=np.float64).ravel()
    expected = np.asarray(expected, dtype=np.float64).ravel()
    n = counts.sum()
    big = expected >= 100.0
    cells = [(int(i), counts[i], expected[i]) for i in np.flatnonzero(big)]
    if (~big).any() and expected[~big].sum() >= 100.0:
        cells.append((-1, counts[~big].sum(), expected[~big].sum()))
    bad = []
    for i, c, e in cells:
        p = e / n
        bound = 6.0 * np.sqrt(max(n * p * (1.0 - p), 0.0))
        if abs(c - e) > bound:
            bad.append((i, c, e, bound))
    return bad


# ---------------------------------------------------------------------------
# the set-up the statistical tests share (tests/test_simulate_reference.py on the oracle, tests/test_simulate_gpu.py
# on the engine): DNA, GTR + G4 + I (p-inv 0.2), 2^20 sites, and the seed that the reference was seen to pass with
# ---------------------------------------------------------------------------
STAT_SITES = 1 << 20
STAT_SEED = 20261020
STAT_PINV = 0.2


def pattern_codes(tips=4, states=4):
    """every column pattern once: uint8 [tips][states^tips], pattern number = sum of state[t] * states^t"""
    n = states ** tips
    idx = np.arange(n)
    return np.stack([(idx // states ** t) % states for t in range(tips)]).astype(np.uint8)


def pattern_instance(lib, pc, tips=4):
    """a partition whose sites are the 4^tips patterns, with the model and tree of the statistical tests"""
    return pc.build_instance(lib, 4, 4, tips, 4 ** tips, pinv=STAT_PINV, codes=pattern_codes(tips), tree=pc.Tree(tips, 52, 53))


def pattern_counts(tip_rows, states=4):
    """counts of the column patterns of uint8 [tips][sites]"""
    tips = tip_rows.shape[0]
    number = np.zeros(tip_rows.shape[1], dtype=np.int64)
    for t in range(tips):
        number += tip_rows[t].astype(np.int64) * states ** t
    return np.bincount(number, minlength=states ** tips)
