"""Substitution mapping on the CPU: tests/substmap_reference.py (numpy.longdouble, bounds derived there) against a
brute-force enumeration of all inner states, the host stage (pllhip_substmap_counts, plain C) against the longdouble
restatement and against quadrature, the identities that tie the tables to the site categories and to the branch
derivative, and the evaluation driver's host path (pllhip_eval_substitution_map on the oracle) against the reference.
The device path is checked against the same reference in tests/test_substmap_gpu.py."""
import itertools

import numpy as np
import pytest

import pllhip_ctypes as pc
import sitecat_reference as sr
import substmap_reference as smr
from test_sitecat_cpu import driver_case

LD = np.longdouble
SITES = pc.PLLHIP_SUBST_SITES


# ---------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------
def conditional(t, P, masks, S, r, node, came_from):
    """the vector of `node` looking away from `came_from`, by pruning in longdouble: [state]"""
    if node < t.ntips:
        return np.array([(masks[node] >> j) & 1 for j in range(S)], dtype=LD)
    out = np.ones(S, dtype=LD)
    for nb, k in t.adj[node]:
        if nb != came_from:
            out = out * (P[k][r] @ conditional(t, P, masks, S, r, nb, node))
    return out


def brute_force_pairs(t, P, masks, S, r, pi, u, v):
    """sum over all assignments of states to ALL nodes (a tip: the states of its mask) of the joint probability of the
    assignment and the data, split by the states (i, j) at u and v: [S][S].  Every edge is read away from u, as the
    definition of J reads them (the engine's fp64 matrices are reversible only to fp64, so the direction is part of it)"""
    nodes = list(range(2 * t.ntips - 2))
    choices = [[j for j in range(S) if (masks[x] >> j) & 1] if x < t.ntips else list(range(S)) for x in nodes]
    root = u                                                # the product starts with the frequency of the state at u
    order, seen, stack = [], {root}, [root]
    while stack:                                            # every edge once, pointing away from `root`
        a = stack.pop()
        for b, k in t.adj[a]:
            if b not in seen:
                seen.add(b)
                order.append((a, b, k))
                stack.append(b)
    out = np.zeros((S, S), dtype=LD)
    for x in itertools.product(*choices):
        joint = pi[x[root]]
        for a, b, k in order:
            joint = joint * P[k][r, x[a], x[b]]
        out[x[u], x[v]] += joint
    return out


BRUTE = [(4, 2, ["0R2", "12-", "301", "0R3", "210"], None, None),
         (4, 2, ["0R2", "02-", "001", "0R3", "000"], [0.3], None),                       # p-inv: sites 0 and 1 have an invariant term
         (4, 2, ["0R2", "02-", "001", "0R3", "000"], [0.2, 0.0], [0, 1]),                # a mixture of two models, one with p-inv
         (3, 1, ["012", "1-0", "201", "002", "210"], None, None),
         (3, 1, ["012", "0-2", "002", "002", "012"], [0.25], None)]


@pytest.mark.parametrize("S,R,seqs,pinv,mixture", BRUTE)
def test_reference_against_brute_force(oracle, S, R, seqs, pinv, mixture):
    """5 tips: J[n][r] of the reference, from vectors pruned here in longdouble towards either end of the edge, is the
    joint posterior of the two end states and the category, from the enumeration of every assignment; on every edge
    kind -- (inner, inner), (inner, tip) and (tip, inner) -- with p-inv and with a mixture"""
    ntips, N = 5, 3
    t = pc.Tree(ntips, 7, 8)
    kw = {"mixture_pinv": pinv} if pinv else {}
    codes = np.zeros((ntips, N), dtype=np.uint8)
    with pc.build_instance(oracle, states=S, rate_cats=R, ntips=ntips, nsites=N, coded=True, tree=t, codes=codes,
                           alpha=0.7, mixture=mixture, **kw) as inst:
        cmap = pc.state_charmap(S)
        if S == 4:
            cmap[ord("R")] = np.uint64(0b0101)
        cmap[ord("-")] = np.uint64((1 << S) - 1)
        for k in range(ntips):
            inst.set_tip_states(k, cmap, seqs[k].encode())
        if pinv:
            assert inst.L.pll_update_invariant_sites(inst.p)
        if R > 1:
            w = pc._f64([0.6, 0.4])
            inst.L.pll_set_category_weights(inst.p, w.ctypes.data_as(pc.c_double_p))
        pc.full_traversal(inst)
        freqs, q, w, rho, m, inv = sr.model_of(inst)
        pi, q, w = np.asarray(freqs, dtype=LD), np.asarray(q, dtype=LD), np.asarray(w, dtype=LD)
        P = [np.asarray(inst.get_pmatrix(k), dtype=LD) for k in range(t.nedges)]
        if pinv:
            assert (inv >= 0).any() and (inv < 0).any()
        edges = [(u, v, k) for k, (u, v) in enumerate(t.edges)] + [(v, u, k) for k, (u, v) in enumerate(t.edges)]
        kinds = set()
        for u, v, k in edges:
            kinds.add((u < ntips, v < ntips))
            parent, child = np.zeros((N, R, S), dtype=LD), np.zeros((N, R, S), dtype=LD)
            want = np.zeros((N, R, S, S), dtype=LD)
            for n in range(N):
                masks = [int(cmap[ord(s[n])]) for s in seqs]
                for r in range(R):
                    parent[n, r] = conditional(t, P, masks, S, r, u, v)
                    child[n, r] = conditional(t, P, masks, S, r, v, u)
                    want[n, r] = w[r] * (1 - q[r]) * brute_force_pairs(t, P, masks, S, r, pi[r], u, v)
                site = want[n].sum() + sum(w[r] * q[r] * pi[r][inv[n]] for r in range(R) if inv[n] >= 0)
                want[n] /= site
            ref = smr.tables(parent, child, P[k], pi, q, w, np.zeros((N, R), dtype=np.int64), inv, m)
            for n in range(N):
                for r in range(R):
                    J = smr.joint(ref, n, r)
                    # both sides in longdouble (unit roundoff 2^-64) from the same matrices read in the same direction,
                    # all terms non-negative.  Roundings on the longest path: the enumeration multiplies 8 factors and
                    # adds at most 4^3 x 8 = 512 assignments (three inner nodes, a gap and a two-state code among the
                    # tips), the site likelihood adds R S^2 entries and R invariant terms and divides: below
                    # 8 + 512 + 34 + 2 = 556; the reference's path (two levels of pruning with 2 S + 1 roundings each,
                    # T with k_T, the quotient and four products) stays below 100: 656 roundings, with the factor 2 of
                    # margin every bound here carries, rounded up: 1400 x 2^-64
                    assert np.all(np.abs(J - want[n, r]) <= LD(1400) * LD(2.0) ** -64 * want[n, r]), (u, v, n, r)
            # ... and the tables are its sums (N = 3 sites, R categories, S^2 entries more: well inside the margin)
            assert np.all(np.abs(ref.pairs - (m[:, None, None, None] * want).sum(axis=0)) <= LD(1400) * LD(2.0) ** -64 * ref.pairs)
            off = want.sum(axis=1) * (1 - np.eye(S, dtype=LD))[None]
            assert np.all(np.abs(ref.differ - off.sum(axis=(1, 2))) <= LD(1400) * LD(2.0) ** -64 * ref.differ)
        assert kinds == {(False, False), (False, True), (True, False)}


# ---------------------------------------------------------------------------
# the host stage
# ---------------------------------------------------------------------------
def random_F(S, seed):
    return (pc.uniform01(seed, S * S) ** 3).reshape(S, S) * 40.0


def model_instance(lib, name):
    """an instance whose partition holds the eigen system of the model: 'gtr', 'protein' (a random reversible 20-state
    model) or 'jc' (three equal eigenvalues)"""
    if name == "protein":
        return pc.build_instance(lib, states=20, rate_cats=1, ntips=4, nsites=2, coded=True)
    inst = pc.build_instance(lib, states=4, rate_cats=1, ntips=4, nsites=2, coded=True)
    if name == "jc":
        inst.set_model([1.0] * 6, [0.25] * 4, np.ones(1))
        inst.L.pll_update_eigen(inst.p, 0)
    return inst


TAUS = [0.0, 1e-9, 0.1, 2.0, 50.0]


@pytest.mark.parametrize("model", ["gtr", "protein", "jc"])
def test_host_stage_against_the_longdouble_restatement(product_nogpu, oracle, model):
    """pllhip_substmap_counts (plain C; the product library without a device and the oracle hold the same file) under
    the derived bound, at tau = 0, 1e-9, 0.1, 2 and 50"""
    worst = 0.0
    with model_instance(oracle, model) as inst:
        pc.full_traversal(inst)
        eig = smr.eigen_of(inst)
        S = inst.S
        if model == "jc":
            lam = np.sort(eig[2])
            assert lam[0] == lam[1] == lam[2] and lam[3] > lam[2]                # the phi(0) branch off the diagonal
        for tau in TAUS:
            F = random_F(S, 5 + int(tau * 10))
            for lib in (product_nogpu, oracle):
                counts, dwell = pc.substmap_counts(lib, *eig, tau, F)
                rc, rd = smr.counts(*eig, tau, F)
                bc, bd = smr.counts_bound(*eig, tau, F)
                if tau == 0.0:
                    assert not counts.any() and not dwell.any()
                assert not np.diag(counts).any()
                fc, fd = np.max(np.abs(counts - rc) / bc), np.max(np.abs(dwell - rd) / bd)
                worst = max(worst, float(fc), float(fd))
                assert fc <= 1.0 and fd <= 1.0, (model, tau, float(fc), float(fd))
                # sum_a dwell[a] = tau sum_ij F o P: all of the time is spent somewhere
                W, V, lm = (np.asarray(x, dtype=LD) for x in eig)
                P = V[:, :S] @ np.diag(np.exp(lm * LD(tau))) @ W[:, :S]
                # (the right-hand side is longdouble; summing S fp64 dwell times adds S - 1 roundings on values whose sum
                # the non-negative tau F o P bounds: S u on top of the entries' own bounds)
                assert abs(dwell.astype(LD).sum() - LD(tau) * (F * P).sum()) <= bd.sum() + S * sr.U * LD(tau) * np.abs(F * P).sum()
    print(f"substmap host stage {model}: worst fraction of the bound {worst:.3f}")


@pytest.mark.parametrize("model", ["gtr", "protein", "jc"])
def test_host_stage_against_quadrature(oracle, model):
    """counts[a][b] = q_ab sum_ij F_ij int_0^tau P_ia(s) P_bj(tau - s) ds and dwell[a] likewise with P_aj, by
    Gauss-Legendre quadrature in longdouble, for tau <= 2.  The tolerance is ten times the quadrature's own error, taken
    as the difference between 32 and 64 nodes, plus the rounding bound.  Measured on the oracle (GTR, the 20-state model
    and JC at tau = 1e-9, 0.1 and 2): the largest difference between 32 and 64 nodes is 3e-17 to 5e-17 of the largest
    entry -- 1.1e-24 against entries of 3.5e-8 at tau = 1e-9, 1.6e-15 against 31.9 at tau = 2 -- which is the fp64
    rounding of leggauss' nodes and weights, not truncation: the integrand is a sum of exponentials with
    |lambda| tau < 7.  The host stage itself stayed below 0.013 of its rounding bound."""
    with model_instance(oracle, model) as inst:
        pc.full_traversal(inst)
        eig = smr.eigen_of(inst)
        S = inst.S
        W, V, lam = (np.asarray(x, dtype=LD) for x in eig)
        W, V = W[:, :S], V[:, :S]
        Q = V @ np.diag(lam) @ W

        def quad(tau, F, nodes):
            x, wts = np.polynomial.legendre.leggauss(nodes)
            M = np.zeros((S, S), dtype=LD)
            for xi, wi in zip(x, wts):
                s = LD(tau) * (LD(xi) + 1) / 2
                Pa = V @ np.diag(np.exp(lam * s)) @ W
                Pb = V @ np.diag(np.exp(lam * (LD(tau) - s))) @ W
                M += LD(wi) * LD(tau) / 2 * (Pa.T @ F @ Pb.T)              # M[a][b] = sum_ij P_ia(s) F_ij P_bj(tau - s)
            c = Q * M
            np.fill_diagonal(c, LD(0))
            return c, np.diag(M).copy()

        for tau in [x for x in TAUS if 0 < x <= 2]:
            F = random_F(S, 9 + int(tau * 10))
            counts, dwell = pc.substmap_counts(oracle, *eig, tau, F)
            (c32, d32), (c64, d64) = quad(tau, F.astype(LD), 32), quad(tau, F.astype(LD), 64)
            qc, qd = np.max(np.abs(c32 - c64)), np.max(np.abs(d32 - d64))
            bc, bd = smr.counts_bound(*eig, tau, F)
            print(f"substmap quadrature {model} tau={tau}: 32 against 64 nodes {float(qc):.3g} / {float(qd):.3g}, "
                  f"largest entries {float(np.max(np.abs(c64))):.3g} / {float(np.max(d64)):.3g}")
            assert np.all(np.abs(counts - c64) <= 10 * qc + bc), (model, tau)
            assert np.all(np.abs(dwell - d64) <= 10 * qd + bd), (model, tau)


# ---------------------------------------------------------------------------
# identities, and the driver on the oracle
# ---------------------------------------------------------------------------
def check_branch(inst, b, flags, worst, where, scale=1.0):
    """one record of the driver against the reference of its edge, read from the partition while the vectors of both ends
    point at each other -- which they do only for the root edge afterwards, so the caller passes records it re-creates"""
    S, R, N = inst.S, inst.R, inst.N
    ref = smr.reference(inst, b.parent, b.parent_scaler, b.child, b.child_scaler, b.matrix)
    fr = smr.worst(b.pairs, ref.pairs, smr.k_pairs(S, R, N), ref.floor_F)
    assert fr <= 1.0, f"{where}: pairs at {fr:.3g} of the bound"
    assert not b.pairs[ref.pairs == 0].any(), where
    if flags:
        fd = smr.worst(b.differ, ref.differ, smr.k_differ(S, R), ref.floor_site)
        assert fd <= 1.0, f"{where}: differ at {fd:.3g} of the bound"
        worst["differ"] = max(worst.get("differ", 0.0), fd)
    else:
        assert b.differ is None
    dF = smr.bound(ref.F, smr.k_F(S, R, N), ref.floor_F)
    c, d, bc, bd = smr.branch(inst, ref, b.length * scale, dF)
    fc, fw = float(np.max(np.abs(b.counts - c) / bc)), float(np.max(np.abs(b.dwell - d) / bd))
    assert fc <= 1.0 and fw <= 1.0, f"{where}: counts / dwell at {fc:.3g} / {fw:.3g} of the bound"
    assert abs(LD(b.total) - c.sum()) <= bc.sum() * (1 + S * S * sr.U)
    assert abs(LD(b.posterior_weight) - ref.posterior.sum()) <= smr.bound(ref.posterior.sum(), smr.k_posterior(S, R, N) + R, ref.floor_F * R * S * S)
    assert b.dropped == ref.dropped
    for k, v in (("pairs", fr), ("counts", fc), ("dwell", fw)):
        worst[k] = max(worst.get(k, 0.0), v)
    # identities: sum_ij pairs[r] = sum_n m_n post[n][r];  sum_a dwell_r[a] = tau_r posterior[r]
    po = sr.posteriors(ref.tab.A, ref.tab.B, ref.tab.c, sr.model_of(inst)[2], None, ref.m)
    want = (ref.m[:, None].astype(LD) * po.post).sum(axis=0)
    assert np.all(np.abs(b.pairs.sum(axis=(1, 2)).astype(LD) - want) <=
                  smr.bound(want, smr.k_posterior(S, R, N) + sr.k_post(S, R), ref.floor_F * S * S))
    tau = smr.taus(inst, b.length * scale)
    # (S - 1 roundings of the fp64 sum over the states, on top of the entries' own bounds)
    assert abs(LD(b.dwell.sum()) - (tau * ref.posterior).sum()) <= bd.sum() + S * sr.U * (tau * ref.posterior).sum()
    return ref


def k_vectors(S, levels=8):
    """what two evaluations of one edge may differ by when their vectors were computed along different traversals: an
    entry of a vector is a sum of non-negative products, 2 S + 3 roundings per level of the tree (two sums of S products,
    their product) and at most `levels` levels below it on a 9-tip tree; the scale holds two vectors in its numerator
    and two in T"""
    return 4 * levels * (2 * S + 3)


def driver_against_reference(lib, states, rate_cats, nsites, linkage, scaler):
    """pllhip_eval_substitution_map of `lib` on a 9-tip tree.  The record of the root edge is held against the reference
    read from the partition afterwards (the walk puts every vector back); for every other branch the driver is
    re-rooted there and the root-edge record of that run is held against the reference, under the derived bounds: so
    every branch of the tree is held against the reference once.  The record the FIRST walk made of that branch (an
    inner vector turned by `reorient`) is the same table from vectors computed along another traversal: both lie within
    k + k_vectors of the exact value, so they differ by at most twice that bound."""
    worst = {}
    ev, inst = driver_case(lib, states, rate_cats, nsites, inputs="ambiguous", pinv=(0.2, 0.1), constant=4)
    S, R, N = states, rate_cats, nsites
    kv = k_vectors(S)
    with ev:
        if linkage:
            ev.set_linkage(1, [scaler])
        before = ev.loglh()
        root = ev.root_edge()
        plain, = ev.substitution_map(0)
        full, = ev.substitution_map(SITES)
        assert ev.root_edge() == root and ev.loglh(incremental=True) == before and ev.loglh() == before
        nb = len(full)
        assert nb == 2 * 9 - 3 and sorted(b.matrix for b in full) == list(range(nb))
        for a, b in zip(plain, full):
            assert a.differ is None and np.array_equal(a.pairs, b.pairs) and np.array_equal(a.counts, b.counts)
        check_branch(inst, full[root[4]], SITES, worst, "root edge", scaler)
        assert (full[root[4]].parent, full[root[4]].child) == (root[0], root[2])
        recs = {}
        for rec in ev.records():
            if rec.contents.next:
                recs.setdefault(rec.contents.pmatrix_index, rec)
        for m, rec in recs.items():
            if m == root[4]:
                continue
            assert ev.L.pllhip_eval_set_root(ev.ev, rec)
            ev.loglh()
            again, = ev.substitution_map(SITES)
            r2 = ev.root_edge()
            ref = check_branch(inst, again[m], SITES, worst, f"branch {m}", scaler)
            first = full[m]
            same = (first.parent, first.child) == (r2[0], r2[2])
            assert same or (first.parent, first.child) == (r2[2], r2[0])
            bd = 2 * smr.bound(ref.differ, smr.k_differ(S, R) + kv, ref.floor_site)
            if same:
                bp = 2 * smr.bound(ref.pairs, smr.k_pairs(S, R, N) + kv, ref.floor_F)
                fp = float(np.max(np.abs(first.pairs - again[m].pairs) / bp))
            else:
                # the other orientation: pairs[i][j] / (pi_i P_ij) = sum_n m s parent_i child_j is the same sum with the
                # two ends exchanged.  (pairs itself is not compared: the engine's fp64 matrices are reversible only
                # to fp64, pi_i P_ij and pi_j P_ji differ in their small entries.)  Three more roundings per side.
                w = ref.pi[:, :, None] * ref.P
                live = w > 0
                x1 = np.where(live, first.pairs.astype(LD) / np.where(live, w, LD(1)), LD(0)).transpose(0, 2, 1)
                x2 = np.where(live, again[m].pairs.astype(LD) / np.where(live, w, LD(1)), LD(0))
                xr = np.where(live, ref.pairs / np.where(live, w, LD(1)), LD(0))
                bp = 2 * smr.bound(xr, smr.k_pairs(S, R, N) + kv + 3, ref.floor_F / np.where(live, w, LD(1)))
                fp = float(np.max(np.abs(x1 - x2) / np.maximum(bp, bp.transpose(0, 2, 1))))
            fd = float(np.max(np.abs(first.differ - again[m].differ) / bd))
            dF = smr.bound(ref.F, smr.k_F(S, R, N) + kv, ref.floor_F)
            _, _, bc, bw = smr.branch(inst, ref, again[m].length * scaler, dF)
            fc = float(np.max(np.abs(first.counts - again[m].counts) / (2 * bc))) if same else 0.0
            fw = float(np.max(np.abs(first.dwell - again[m].dwell) / (2 * bw))) if same else 0.0
            ft = float(abs(LD(first.total) - LD(again[m].total)) / (2 * bc.sum()))
            for k, v in (("walk pairs", fp), ("walk differ", fd), ("walk counts", fc), ("walk dwell", fw), ("walk total", ft)):
                worst[k] = max(worst.get(k, 0.0), v)
            assert max(fp, fd, fc, fw, ft) <= 1.0, (m, fp, fd, fc, fw, ft)
    print(f"substmap driver S={states} linkage={linkage}: worst fractions of the bounds {worst}")
    return worst


DRIVER = [(4, 4, 0, 1.0), (20, 4, 0, 1.0), (4, 4, 1, 0.7), (20, 4, 1, 1.3)]


@pytest.mark.parametrize("states,rate_cats,linkage,scaler", DRIVER)
def test_driver_on_the_oracle_against_the_reference(oracle, states, rate_cats, linkage, scaler):
    """linked and scaled lengths, with differ on request; root and log-likelihood are what they were"""
    driver_against_reference(oracle, states, rate_cats, 33, linkage, scaler)


def test_unknown_flags_and_no_local_partition_are_refused(oracle):
    ev, inst = driver_case(oracle, 4, 4, 33)
    with ev:
        with pytest.raises(RuntimeError):
            ev.substitution_map(2)
    tree = pc.Tree(9, 42, 43)
    with pc.Evaluation(oracle, tree.newick(), nparts=1) as empty:
        empty.add_remote_partition(0)
        with pytest.raises(RuntimeError):
            empty.substitution_map(0)


@pytest.mark.parametrize("states", [4, 20])
def test_derivative_identity_on_the_oracle(oracle, states):
    """sum_r sum_ij F_r o dP_r/dt is the first derivative of the log-likelihood along the edge:
    pll_compute_likelihood_derivatives returns the derivatives of -lnL, hence the sign.  The sum is signed, so the
    difference is held against the sum of the absolute terms (state space and the eigen basis of the sumtable), times
    2 (4 S + N + k_T + 20) u: the roundings of the reference's F (k_F), of dP (two products of length S) and of the
    oracle's sumtable scan (two products of length S, the exponentials, the quotient by the site likelihood)."""
    from test_ancestral_exact import build_case
    with build_case(oracle, states, 4, 33, True) as inst:
        t = inst.tree
        for parent, child, m in ((t.parent, t.child, t.m_inner), (t.root_a, t.root_b, t.root_matrix)):
            ref = smr.reference(inst, parent, t.scaler_of(parent), child, t.scaler_of(child), m)
            st = inst.alloc_sumtable()
            inst.update_sumtable(parent, child, t.scaler_of(parent), t.scaler_of(child), st)
            df, _ = inst.derivatives(t.scaler_of(parent), t.scaler_of(child), float(t.brlens[m]), st)
            inst.free_sumtable(st)
            total, cond = smr.derivative(inst, ref, float(t.brlens[m]))
            k = 4 * states + 33 + sr.k_T(states, 4) + 20
            assert abs(LD(-df) - total) <= LD(2 * k) * sr.U * cond, (m, df, float(total), float(cond))
