"""Neighbour joining by the rules of INTEGRATION.md, "Pairwise distances and neighbour joining", restated in numpy: what
pllhip_distmat_nj_joins must return bit for bit.  Every operation is one IEEE double operation in the order written
(numpy does not contract), the arg-min breaks ties towards the smallest (i, j), and the row sums are made in ascending
order of k (a cumulative sum, not numpy's pairwise sum)."""
import numpy as np


def nj(matrix):
    """(slots uint32 [2 (T - 3) + 3], lengths float64 [2 (T - 3) + 3]): per round (i, j) and (l_i, l_j), then the
    last three slots and their lengths; not clamped"""
    d = np.array(matrix, dtype=np.float64)
    T = d.shape[0]
    assert d.shape == (T, T) and T >= 3
    r = np.cumsum(d, axis=1)[:, -1].copy()
    alive = np.arange(T)
    slots, lengths = [], []
    for n in range(T, 3, -1):
        sub = d[np.ix_(alive, alive)]
        ra = r[alive]
        q = (np.float64(n - 2) * sub - ra[:, None]) - ra[None, :]
        q[np.tril_indices(n)] = np.inf
        a, b = np.argwhere(q == q.min())[0]                # row-major: the smallest (i, j) of the smallest value
        i, j = alive[a], alive[b]
        dij, ri, rj = d[i, j], r[i], r[j]
        li = dij / 2.0 + (ri - rj) / (2.0 * (np.float64(n) - 2.0))
        lj = dij - li
        slots += [i, j]
        lengths += [li, lj]
        others = alive[(alive != i) & (alive != j)]
        dik, djk = d[i, others].copy(), d[j, others].copy()
        duk = ((dik + djk) - dij) / 2.0
        r[others] = ((r[others] - dik) - djk) + duk
        r[i] = ((ri + rj) - np.float64(n) * dij) / 2.0
        d[i, others] = duk
        d[others, i] = duk
        alive = alive[alive != j]
    a, b, c = alive
    slots += [a, b, c]
    lengths += [((d[a, b] + d[a, c]) - d[b, c]) / 2.0, ((d[a, b] + d[b, c]) - d[a, c]) / 2.0,
                ((d[a, c] + d[b, c]) - d[a, b]) / 2.0]
    return np.array(slots, dtype=np.uint32), np.array(lengths, dtype=np.float64)


def _normal(side, T):
    side = frozenset(int(x) for x in side)
    return side if 0 not in side else frozenset(range(T)) - side


def splits_of_joins(T, slots):
    """the splits of the joined tree, trivial ones included, each as the side without tip 0 (what
    pllhip_ctypes.utree_splits gives for a tree whose tips are 0 .. T - 1)"""
    below = {s: frozenset([s]) for s in range(T)}
    out = {_normal([s], T) for s in range(T)}
    for q in range(T - 3):
        i, j = int(slots[2 * q]), int(slots[2 * q + 1])
        below[i] = below[i] | below[j]
        out.add(_normal(below[i], T))
    return out


def random_tree(T, rng, lo=0.05, hi=0.3):
    """a random binary unrooted tree over tips 0 .. T - 1 with branch lengths in [lo, hi): (path-length matrix, splits)"""
    edges = [[0, T], [1, T], [2, T]]
    for t in range(3, T):
        e = int(rng.integers(len(edges)))
        u, v = edges[e]
        w = T + t - 2
        edges[e] = [u, w]
        edges += [[w, v], [t, w]]
    lengths = rng.uniform(lo, hi, size=len(edges))
    nodes = 2 * T - 2
    adj = [[] for _ in range(nodes)]
    for k, (u, v) in enumerate(edges):
        adj[u].append((v, k))
        adj[v].append((u, k))
    dist = np.zeros((T, T))
    for s in range(T):
        depth = np.full(nodes, -1.0)
        depth[s] = 0.0
        stack = [s]
        while stack:
            u = stack.pop()
            for v, k in adj[u]:
                if depth[v] < 0.0:
                    depth[v] = depth[u] + lengths[k]
                    stack.append(v)
        dist[s] = depth[:T]
    dist = (dist + dist.T) / 2.0                          # (the two directions add the same lengths in another order)
    np.fill_diagonal(dist, 0.0)
    splits = set()
    for k, (u, v) in enumerate(edges):                    # the tips on v's side of edge k
        seen, stack = {u, v}, [v]
        side = set()
        while stack:
            x = stack.pop()
            if x < T:
                side.add(x)
            for y, _ in adj[x]:
                if y not in seen:
                    seen.add(y)
                    stack.append(y)
        splits.add(_normal(side, T))
    return dist, splits
