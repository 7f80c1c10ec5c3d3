"""The contract of pllhip_sample_ancestral_edges ("Sampled ancestral states") restated in numpy float64,
vectorised over the sites, for tests only.  It is fed with what the library under test holds -- its vectors (a coded tip
as the 0/1 expansion of its masks), its P-matrices, the site-category table of the root edge, frequencies, weights and
invariant states -- and runs the same operations in the same order, so its bytes are the library's bytes: the tests
compare with ==, no tolerance and no excluded draws.

    masses of a site          m[2r] = w_r A[n][r],  m[2r+1] = w_r B[n][r]                        (stream 0)
    root state, category r    omega_i = (pi_r[i] root[n,r,i]) t_i,  t_i = sum_j P_r^m0[i][j] other[n,r,j]   (stream 2)
    edge parent -> child      omega_j = P_r^m[a][j] child[n,r,j],  a the parent's state          (stream 3 + m)

Every table is cumulated left to right, one add after the other (an explicit loop, not numpy.cumsum, whose pairwise
blocks add in another order); x = u total is one multiply; the pick is the bisection of sim_pick.  u(b, k, n) and mix
are those of tests/simulate_reference.py.  A site whose total mass is not > 0 or not finite is dropped: 0xFF everywhere.

The table comes from the library: `device_table` reads pllhip_sitecat_table of the root edge; `host_table` restates, in
float64 and in its order of operations, the table the evaluation driver forms on the host where the library has no
device call (the CPU oracle).

The rounding bound of the formula test (`formula_bound`).  The test multiplies the three conditional probabilities of
one joint assignment (component, root state, other inner state) of a four-tip tree and compares with the exact posterior
from the library's P-matrices in longdouble.  With u = 2^-53, S states, R categories, counting roundings on the longest
path (sums of non-negative terms: relative errors do not grow in a sum):
    an inner vector element     k_v = 2 S              S products, S - 1 additions per child, one product
    a table entry A             k_A = (2 S + 8) + 2 k_v   sitecat_reference.k_tab, and both vectors' own errors
    a component mass            k_m = k_A + 1
    factor 1, m_k / total       k_1 = 2 k_m + 2 R + 1     the total adds 2 R - 1 roundings, the quotient one
    a root mass omega_i         k_w = (2 S + 1) + 2 k_v   t_i: 2 S - 1 and other's error; two products; root's error
    factor 2                    k_2 = 2 k_w + S
    an edge mass                k_e = 1 + k_v
    factor 3                    k_3 = 2 k_e + S
    their product               K = k_1 + k_2 + k_3 + 2
The bound is 2 K u relative (a factor 2 of margin, which also covers the longdouble side)."""
import numpy as np

import ancestral_reference as ar
import pllhip_ctypes as pc
import simulate_reference as simr
import sitecat_reference as sr

_U = np.uint64
RATE_MAXDIFF = 4


def formula_bound(S, R):
    k_v = 2 * S
    k_m = (2 * S + 8) + 2 * k_v + 1
    k_1 = 2 * k_m + 2 * R + 1
    k_2 = 2 * ((2 * S + 1) + 2 * k_v) + S
    k_3 = 2 * (1 + k_v) + S
    return 2.0 * (k_1 + k_2 + k_3 + 2) * 2.0 ** -53


def cumulate(x):
    """running sums along the last axis from 0.0, one add after the other; nothing is clamped"""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    acc = np.zeros(x.shape[:-1])
    for s in range(x.shape[-1]):
        acc = acc + x[..., s]
        out[..., s] = acc
    return out


def pick(u, cum):
    """x = u total, then the bisection of sim_pick row by row: u [N], cum [N][n] -> [N]"""
    n = cum.shape[-1]
    x = u * cum[:, -1]
    rows = np.arange(len(cum))
    lo, hi = np.zeros(len(cum), dtype=np.int64), np.full(len(cum), n - 1, dtype=np.int64)
    while (lo < hi).any():
        act = lo < hi
        mid = (lo + hi) >> 1
        above = cum[rows, mid] > x
        hi = np.where(act & above, mid, hi)
        lo = np.where(act & ~above, mid + 1, lo)
    return lo


def device_table(inst, root_edge, matrix):
    """(A, B) [site][cat] float64 of pllhip_sitecat_table for the root edge (root node, root scaler, other, other scaler)"""
    with pc.SiteCat.edge(inst, root_edge[0], root_edge[1], root_edge[2], root_edge[3], matrix) as sc:
        A, B, _ = sc.table()
    return A, B


def host_table(inst, root_edge, matrix):
    """(A, B) of the driver's host table (pllhip_eval.c, sc_host_table) in float64, operation for operation"""
    rn, rs, on, os_ = root_edge
    freqs, q, w, rho, m, inv = sr.model_of(inst)
    parent, child, P = ar.clv_of(inst, rn), ar.clv_of(inst, on), inst.get_pmatrix(matrix)
    counts = sr.counts_of(inst, rs) + sr.counts_of(inst, os_)
    N, R, S = parent.shape
    cnt = counts.min(axis=1)
    has = inv >= 0
    binv = np.zeros(N)
    for r in range(R):
        if q[r] > 0:
            binv[has] += w[r] * q[r] * freqs[r][inv[has]]
    descale = (binv > 0) & (cnt > 0)
    A, B = np.zeros((N, R)), np.zeros((N, R))
    for r in range(R):
        l = np.zeros(N)
        for i in range(S):
            a = np.zeros(N)
            for j in range(S):
                a = a + P[r, i, j] * child[:, r, j]
            l = l + (freqs[r][i] * parent[:, r, i]) * a
        d = np.minimum(counts[:, r] - cnt, RATE_MAXDIFF)
        l = np.where(d > 0, l * 2.0 ** (-256.0 * d), l)
        l = np.where(descale, np.where(cnt <= 3, l * 2.0 ** (-256.0 * np.minimum(cnt, 3)), 0.0), l)
        A[:, r] = (1.0 - q[r]) * l if q[r] > 0 else l
        if q[r] > 0:
            B[has, r] = q[r] * freqs[r][inv[has]]
    return A, B


class Inputs:
    """what one call reads: A, B [N][R]; w [R]; freqs [R][S] (through freqs_indices); invariant [N] (-1: none);
    m [N] pattern weights; clv: node -> [N][R][S]; pmat: matrix index -> [R][S][S]; root, other, m0; edges
    (parent, child, matrix); tips; node_count"""

    def comp_mass(self):
        N, R = self.A.shape
        out = np.zeros((N, 2 * R))
        out[:, 0::2] = self.w[None, :] * self.A
        out[:, 1::2] = self.w[None, :] * self.B
        return out

    def root_mass(self, r):
        """omega [N][S] for the categories r [N]"""
        rows = np.arange(len(r))
        P0, root, other = self.pmat[self.m0], self.clv[self.root][rows, r], self.clv[self.other][rows, r]
        S = root.shape[1]
        t = np.zeros((len(r), S))
        for j in range(S):
            t = t + P0[r, :, j] * other[:, j][:, None]
        return (self.freqs[r] * root) * t

    def edge_mass(self, child, matrix, r, a):
        """omega [N][S] for the categories r [N] and the parent's states a [N]"""
        rows = np.arange(len(r))
        return self.pmat[matrix][r, a] * self.clv[child][rows, r]


def gather(inst, tree_edges, root_edge, table, node_count=None):
    """the Inputs of a call on `inst`: tree_edges = (parent, child, matrix) arrays, root_edge = (root node, root scaler,
    other node, other scaler), table = device_table or host_table"""
    x = Inputs()
    parent, child, matrix = (np.asarray(a, dtype=np.int64) for a in tree_edges)
    x.edges = list(zip(parent.tolist(), child.tolist(), matrix.tolist()))
    x.root, x.other = int(root_edge[0]), int(root_edge[2])
    x.m0 = next(m for p, c, m in x.edges if p == x.root and c == x.other)
    x.A, x.B = table(inst, root_edge, x.m0)
    freqs, q, w, rho, m, inv = sr.model_of(inst)
    x.freqs, x.w, x.m, x.invariant = freqs, w, m, inv
    x.clv = {n: ar.clv_of(inst, n) for n in {x.root} | set(child.tolist())}
    x.pmat = {k: inst.get_pmatrix(k) for k in set(matrix.tolist())}
    x.tips = inst.tips
    x.node_count = inst.tips + inst.p.contents.clv_buffers if node_count is None else node_count
    return x


def sample(x, seed, replicates, first_replicate=0, tips=False, alphabet=None):
    """(out uint8 [replicates][node_count][N], component uint8 [replicates][N], dropped)"""
    N, R = x.A.shape
    n = np.arange(N, dtype=_U)
    out = np.full((replicates, x.node_count, N), 255, dtype=np.uint8)
    comp = np.full((replicates, N), 255, dtype=np.uint8)
    cumc = cumulate(x.comp_mass())
    total = cumc[:, -1]
    live = (total > 0) & np.isfinite(total)
    dropped = int((~live & (x.m > 0)).sum())
    kids = {}
    for p, c, m in x.edges:
        kids.setdefault(p, []).append((c, m))
    table = None if alphabet is None else np.frombuffer(alphabet if isinstance(alphabet, bytes) else alphabet.encode(), np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(replicates):
            b = first_replicate + i
            k = pick(simr.uniform(seed, b, 0, n), cumc)
            r, inv = k >> 1, (k & 1) == 1
            comp[i] = np.where(live, r | (inv.astype(np.int64) << 7), 255).astype(np.uint8)
            inv_state = x.invariant & 255
            state = {x.root: np.where(inv, inv_state, pick(simr.uniform(seed, b, 2, n), cumulate(x.root_mass(r))))}
            order = [x.root]
            for node in order:
                for child, m in kids.get(node, ()):
                    a = np.where(inv, 0, state[node])
                    drawn = pick(simr.uniform(seed, b, 3 + m, n), cumulate(x.edge_mass(child, m, r, a)))
                    state[child] = np.where(inv, inv_state, drawn)
                    order.append(child)
            for node, s in state.items():
                if node >= x.tips or tips:
                    byte = s.astype(np.int64)
                    if table is not None:
                        byte = np.where(byte == 255, 255, table[np.minimum(byte, len(table) - 1)])
                    out[i, node] = np.where(live, byte, 255).astype(np.uint8)
    return out, comp, dropped


def driver_edges(ev):
    """the edge list the evaluation driver walks: ((parent, child, matrix) arrays, parents first and the root edge
    first, (root node, root scaler, other node, other scaler)) from the driver's root record, seen from its inner end"""
    import ctypes as C
    root = ev.L.pllhip_eval_root(ev.ev)
    if not root.contents.next:
        root = root.contents.back
    addr = lambda rec: C.addressof(rec.contents)
    parent, child, matrix, stack = [], [], [], [root]
    while stack:
        entry = stack.pop()
        n = entry if addr(entry) == addr(root) else entry.contents.next
        if not n:
            continue
        first = addr(n) if addr(entry) == addr(root) else addr(entry)
        while True:
            parent.append(n.contents.clv_index)
            child.append(n.contents.back.contents.clv_index)
            matrix.append(n.contents.pmatrix_index)
            stack.append(n.contents.back)
            n = n.contents.next
            if addr(n) == first:
                break
    r, b = root.contents, root.contents.back.contents
    return (np.array(parent), np.array(child), np.array(matrix)), (r.clv_index, r.scaler_index, b.clv_index, b.scaler_index)
