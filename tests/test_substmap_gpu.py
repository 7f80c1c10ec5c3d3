"""The pair-table kernels (kernels_substmap.hpp; pllhip_substmap_edge) and the whole-tree driver on the device against
tests/substmap_reference.py: F, pairs, posterior and differ in numpy.longdouble from what the engine itself holds, under
the bounds derived there.  The reference excludes nothing: every entry of every table is held against it, and entries
that are exactly zero there are zero here."""
import numpy as np
import pytest

import pllhip_ctypes as pc
import sitecat_reference as sr
import substmap_reference as smr
from test_ancestral_exact import build_case, triples_of
from test_sitecat_cpu import driver_case
from test_substmap_cpu import driver_against_reference, k_vectors
from test_sitecat_gpu import KERNELS, SHAPES, SITES, edge_of, unequal_weights

LD = np.longdouble
WITH_SITES = pc.PLLHIP_SUBST_SITES
FIELDS = ("F", "pairs", "posterior", "differ")


def within(worst, name, got, ref, k, floor, where):
    frac = smr.worst(got, ref, k, floor)
    print(f"  {where}: {name} at {frac:.4f} of its bound")
    worst[name] = max(worst.get(name, 0.0), frac)
    assert frac <= 1.0, f"{where}: {name} is {frac:.3g} of its bound"
    zero = np.asarray(ref) == 0
    assert not np.asarray(got)[zero].any(), f"{where}: {name} is not zero where the reference is"
    return int(zero.sum())


def check_edge(inst, triple, worst, where, flags=WITH_SITES):
    """one call, twice (every array repeats bit for bit), against the reference of the edge"""
    S, R, N = inst.S, inst.R, inst.N
    edge = edge_of(inst, triple)
    ref = smr.reference(inst, *edge)
    with pc.EdgePairs.edge(inst, *edge, flags) as got, pc.EdgePairs.edge(inst, *edge, flags) as again:
        assert (got.states, got.cats, got.sites) == (S, R, N)
        for f in FIELDS:
            assert np.array_equal(getattr(got, f), getattr(again, f)), (where, f)
        assert (got.dropped, got.weight_sum) == (again.dropped, again.weight_sum)
    zeros = within(worst, "F", got.F, ref.F, smr.k_F(S, R, N), ref.floor_F, where)
    within(worst, "pairs", got.pairs, ref.pairs, smr.k_pairs(S, R, N), ref.floor_F, where)
    within(worst, "posterior", got.posterior, ref.posterior, smr.k_posterior(S, R, N), ref.floor_F * S * S, where)
    if flags:
        zeros += within(worst, "differ", got.differ, ref.differ, smr.k_differ(S, R), ref.floor_site, where)
    else:
        assert got.differ is None
    assert got.dropped == ref.dropped and got.weight_sum == float(ref.m.sum()), where
    return got, ref, zeros


@pytest.mark.gpu
@pytest.mark.parametrize("coded", [True, False], ids=["coded", "tip-vectors"])
@pytest.mark.parametrize("states,rate_cats", SHAPES)
def test_every_kernel_at_every_site_count(product, states, rate_cats, coded):
    """all four operand kinds (inner x inner, inner x tip, tip x inner, tip x tip, adjacent and not), a zero-length and a
    length-50 matrix; N = 1, 2, 31, 32, 33, 64, 130: an empty tail, an odd tail, a full block, a second wave, a second
    workgroup.  Tips that disagree across the zero-length matrix give all-zero tables and dropped sites."""
    worst, zeros, dropped = {}, 0, 0
    for nsites in SITES:
        with build_case(product, states, rate_cats, nsites, coded) as inst:
            assert product.lib.pllhip_partials_kernel_name(inst.p) == KERNELS[states, rate_cats]
            unequal_weights(inst)
            for k, triple in enumerate(triples_of(inst.tree)):
                got, ref, z = check_edge(inst, triple, worst, f"N={nsites} entry {k} {triple}")
                zeros += z
                dropped += got.dropped
    print(f"substmap S={states} R={rate_cats} coded={coded}: worst fractions of the bounds {worst}; {zeros} zero entries, "
          f"{dropped} dropped sites")
    assert zeros > 0 and dropped > 0


VARIANTS = [(S, R, v) for S, R in SHAPES for v in ("pinv", "mixture", "ambiguous-pinv") if R > 1 or v == "pinv"]


@pytest.mark.gpu
@pytest.mark.parametrize("states,rate_cats,variant", VARIANTS)
def test_pinv_mixture_and_ambiguity_codes(product, states, rate_cats, variant):
    worst = {}
    kw = {"pinv": {"mixture_pinv": [0.25]}, "mixture": {}, "ambiguous-pinv": {"mixture_pinv": [0.3, 0.0]}}[variant]
    inputs = {"pinv": "plain", "mixture": "mixture", "ambiguous-pinv": "ambiguous"}[variant]
    for nsites in (33, 130):
        for coded in (True, False):
            with build_case(product, states, rate_cats, nsites, coded, inputs, **kw) as inst:
                if variant != "mixture":
                    assert inst.p.contents.invariant
                unequal_weights(inst)
                for k, triple in enumerate(triples_of(inst.tree)):
                    check_edge(inst, triple, worst, f"{variant} N={nsites} coded={coded} entry {k}")
                check_edge(inst, triples_of(inst.tree)[0], worst, f"{variant} without differ", flags=0)
    print(f"substmap S={states} R={rate_cats} {variant}: worst fractions of the bounds {worst}")


DEEP = [(4, 300, 4), (20, 300, 4), (61, 100, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("attributes", [0, pc.PLL_ATTRIB_RATE_SCALERS], ids=["site-scalers", "rate-scalers"])
@pytest.mark.parametrize("states,ntips,rate_cats", DEEP)
def test_scaled_vectors(product, states, ntips, rate_cats, attributes):
    """a deep tree with long branches (the scaled cases of tests/test_sitecat_gpu.py, with the branch lengths of
    tests/test_sitecat_cpu.py's deep cases, under which constant sites are scaled too): scaler counts on both sides of an
    edge, per site and per (site, rate); the first eight sites are constant, so with p-inv they have an invariant term,
    and some of them c > 0: their scale carries 2^(-256 c), or 0 beyond c = 3"""
    worst = {}
    tree = pc.Tree(ntips, 42, 43)
    tree.brlens = tree.brlens * 40.0
    codes = pc.random_codes(ntips, 65, states, 44)
    codes[:, :8] = (np.arange(8) % states)[None, :]
    with pc.build_instance(product, states=states, rate_cats=rate_cats, ntips=ntips, nsites=65, coded=True, tree=tree,
                           codes=codes, alpha=2.0, attributes=attributes,
                           mixture_pinv=[0.2]) as inst:
        pc.full_traversal(inst)
        unequal_weights(inst)
        top = tree.ops[-1]
        child, m = next((c, k) for c, k in ((top[2], top[3]), (top[5], top[6])) if c >= ntips)
        assert inst.get_scaler(tree.scaler_of(tree.root_a)).any() and inst.get_scaler(tree.scaler_of(child)).any()
        counts = sr.counts_of(inst, tree.scaler_of(tree.root_a)) + sr.counts_of(inst, tree.scaler_of(child))
        assert counts[:8].min(axis=1).any() and (sr.model_of(inst)[5][:8] >= 0).all()      # invariant term and c > 0
        for k, triple in enumerate([(tree.root_a, child, m), (child, tree.root_a, m),
                                    (tree.root_a, tree.root_b, tree.root_matrix),
                                    (tree.root_b, tree.root_a, tree.root_matrix)]):
            got, ref, _ = check_edge(inst, triple, worst, f"{ntips} tips entry {k}")
            assert not ref.tab.c[:8].any()
    print(f"substmap S={states} deep tree, attributes {attributes}: worst fractions of the bounds {worst}")


@pytest.mark.gpu
@pytest.mark.parametrize("states,rate_cats", [(4, 4), (5, 4), (20, 4), (61, 4), (20, 16)])
def test_block_caps(product, monkeypatch, states, rate_cats):
    """PLLHIP_SUBSTMAP_BLOCKS = 1, 2, 3 at 130 sites: a wave walks several blocks, a workgroup several chunks.  differ
    does not depend on the cap; F is another order of summation, within the bound of the reference either way, hence
    within twice the bound of the uncapped run; two runs at one cap agree bit for bit."""
    with build_case(product, states, rate_cats, 130, True, "ambiguous", mixture_pinv=[0.2, 0.1]) as inst:
        unequal_weights(inst)
        S, R, N = inst.S, inst.R, inst.N
        for triple in triples_of(inst.tree)[:3]:
            monkeypatch.delenv("PLLHIP_SUBSTMAP_BLOCKS", raising=False)
            free, ref, _ = check_edge(inst, triple, {}, f"uncapped {triple}")
            for cap in (1, 2, 3):
                monkeypatch.setenv("PLLHIP_SUBSTMAP_BLOCKS", str(cap))
                capped, _, _ = check_edge(inst, triple, {}, f"cap {cap} {triple}")       # (twice, bit for bit, in there)
                assert np.array_equal(capped.differ, free.differ), (cap, triple)
                assert np.all(np.abs(capped.F.astype(LD) - free.F) <= 2 * smr.bound(ref.F, smr.k_F(S, R, N), ref.floor_F))
            monkeypatch.delenv("PLLHIP_SUBSTMAP_BLOCKS", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("states", [4, 20])
def test_derivative_identity_on_the_device(product, states):
    """sum_r sum_ij F_r o dP_r/dt against the engine's own pll_compute_likelihood_derivatives (derivatives of -lnL) on the
    same edge; the bound of tests/test_substmap_cpu.py::test_derivative_identity_on_the_oracle, with the device's F in
    place of the reference's (its own k_F on the absolute terms)"""
    with build_case(product, states, 4, 130, True) as inst:
        t = inst.tree
        N = inst.N
        for parent, child, m in ((t.parent, t.child, t.m_inner), (t.root_a, t.root_b, t.root_matrix)):
            edge = (parent, t.scaler_of(parent), child, t.scaler_of(child), m)
            ref = smr.reference(inst, *edge)
            with pc.EdgePairs.edge(inst, *edge) as got:
                F = got.F.astype(LD)
            st = inst.alloc_sumtable()
            inst.update_sumtable(parent, child, edge[1], edge[3], st)
            df, _ = inst.derivatives(edge[1], edge[3], float(t.brlens[m]), st)
            inst.free_sumtable(st)
            total, cond = smr.derivative(inst, ref, float(t.brlens[m]))
            ref.F = F
            mine, _ = smr.derivative(inst, ref, float(t.brlens[m]))
            k = 4 * states + N + sr.k_T(states, 4) + 20
            print(f"  S={states} matrix {m}: -df {-df:.12g}, sum F o dP {float(mine):.12g}, conditioning {float(cond):.3g}")
            assert abs(LD(-df) - mine) <= LD(2 * (k + smr.k_F(states, 4, N))) * sr.U * cond, (m, df, float(mine))
            assert abs(mine - total) <= LD(2 * smr.k_F(states, 4, N)) * sr.U * cond


@pytest.mark.gpu
@pytest.mark.parametrize("states,linkage,scaler", [(4, 0, 1.0), (20, 0, 1.0), (4, 1, 0.7), (20, 1, 1.3)])
def test_whole_tree_against_the_reference(product, states, linkage, scaler):
    """pllhip_eval_substitution_map on the device, 9 tips, 130 sites, every branch held against the reference read from
    the device's own partition under the derived bounds, nothing added (tests/test_substmap_cpu.py,
    driver_against_reference: what the oracle's driver is held to)"""
    driver_against_reference(product, states, 4, 130, linkage, scaler)


def matrix_difference_cap(eig_a, eig_b, tau, S):
    """how far the fp64 transition matrices of two engines may lie apart, per entry: each engine evaluates the signed eigen
    sum P_ij = sum_k V_ik e^(lambda_k tau) W_kj of ITS OWN eigen system with S products of three factors, an exponential
    (an ulp, and the rounding of lambda tau magnified by |lambda| tau) and S - 1 additions, so it lies within
    (2 S + 8 + max|lambda| tau) u sum_k |V_ik| e^(lambda_k tau) |W_kj| of that sum; the two exact sums differ by what
    the two eigen systems differ by, which is computed here in longdouble.  With the factor 2 of margin of every bound."""
    exact, cond = [], []
    for W, V, lam in (eig_a, eig_b):
        W, V, lam = np.asarray(W, dtype=LD)[:, :S], np.asarray(V, dtype=LD)[:, :S], np.asarray(lam, dtype=LD)
        e = np.exp(lam * tau)
        exact.append(V @ np.diag(e) @ W)
        cond.append(LD(2 * S + 8 + float(np.max(np.abs(lam)) * tau)) * sr.U * (np.abs(V) @ np.diag(e) @ np.abs(W)))
    return 2 * (np.abs(exact[0] - exact[1]) + cond[0] + cond[1])


@pytest.mark.gpu
@pytest.mark.parametrize("states", [4, 20])
def test_whole_tree_against_the_oracle(product, oracle, states):
    """pllhip_eval_substitution_map on the device against the same driver on the oracle (host path), 9 tips, 130 sites,
    every branch, under the sum of the two bounds -- and of what the two engines' inputs differ by, because they do not
    hold the same inputs: their transition matrices come from different code and different eigen decompositions, and a
    small entry of a signed eigen sum differs by far more than a rounding.  That difference is not taken as found: it is
    capped by matrix_difference_cap (the conditioning of each engine's eigen sum plus the exact difference of the two
    eigen systems), the measured difference is asserted to stay under the cap, and rP is the largest cap over an entry,
    in units of u.  A vector entry is a sum of non-negative products over at most 8 levels, each with 2 S + 3 roundings
    (k_vectors) and two matrix entries, the scale holds two vectors in its numerator and two in T, and the pair table has
    one more matrix entry of its own: k_vectors + 4 x 8 x 2 rP + rP is added to every k.  The unwidened check of the
    device's driver is test_whole_tree_against_the_reference."""
    R, N = 4, 130
    out = []
    for lib in (product, oracle):
        ev, inst = driver_case(lib, states, R, N, inputs="ambiguous", pinv=(0.2, 0.1), constant=4)
        with ev:
            before = ev.loglh()
            got, = ev.substitution_map(WITH_SITES)
            assert ev.loglh(incremental=True) == before
            _, persite = ev.persite_lnl(0)
            out.append((got, persite, sr.model_of(inst)[4], [smr.eigen_of(inst, int(inst.params[r])) for r in range(R)],
                        smr.taus(inst, 1.0), np.array([inst.get_pmatrix(k) for k in range(len(got))])))
    (dev, _, _, eig_d, _, Pd), (orc, persite, m, eig, speed, Po) = out
    assert np.array_equal(Pd > 0, Po > 0)
    rP, seen, used = 0.0, 0.0, 0.0
    for k, b in enumerate(orc):
        for r in range(R):
            cap = matrix_difference_cap(eig_d[r], eig[r], speed[r] * LD(b.length), states)
            live = Po[k, r] > 0
            diff = np.abs(Pd[k, r].astype(LD) - Po[k, r])
            used = max(used, float(np.max(diff / cap)))
            seen = max(seen, float(np.max(diff[live] / (sr.U * Po[k, r][live]))))
            rP = max(rP, float(np.max(cap[live] / (sr.U * Po[k, r][live]))))
    print(f"  S={states}: the matrices of the two engines differ by up to {seen:.1f} u relative, {used:.4f} of the cap; "
          f"the cap allows {rP:.1f} u")
    assert used <= 1.0
    kv = k_vectors(states) + 4 * 8 * 2 * rP + rP
    floor_site = smr.TINY * (1 + np.exp(-persite.astype(LD)))
    floor_F = (m.astype(LD) * floor_site).sum()
    worst = {}
    for a, b in zip(dev, orc):
        assert (a.parent, a.child, a.matrix, a.dropped) == (b.parent, b.child, b.matrix, b.dropped)
        bp = 2 * smr.bound(b.pairs, smr.k_pairs(states, R, N) + kv, floor_F)
        bd = 2 * smr.bound(b.differ, smr.k_differ(states, R) + kv, floor_site)
        fp, fd = float(np.max(np.abs(a.pairs - b.pairs) / bp)), float(np.max(np.abs(a.differ - b.differ) / bd))
        bc, bw = np.zeros((states, states), dtype=LD), np.zeros(states, dtype=LD)
        # the host stage at the oracle's F_r = pairs_r / P_r (every branch of this tree is longer than 0, so P > 0),
        # with the bound of F as its dF
        dF_rel = LD(2 * 2 * (smr.k_F(states, R, N) + kv)) * sr.U
        for r in range(R):
            tau = speed[r] * LD(b.length)
            W, V, lam = (np.asarray(x, dtype=LD) for x in eig[r])
            Pm = V[:, :states] @ np.diag(np.exp(lam * tau)) @ W[:, :states]
            Fr = np.where(Pm > 0, b.pairs[r].astype(LD) / np.where(Pm > 0, Pm, LD(1)), LD(0))
            c1, d1 = smr.counts_bound(*eig[r], tau, Fr, dF_rel * Fr + floor_F)
            bc, bw = bc + 2 * c1, bw + 2 * d1
        fc, fw = float(np.max(np.abs(a.counts - b.counts) / bc)), float(np.max(np.abs(a.dwell - b.dwell) / bw))
        for k, v in (("pairs", fp), ("differ", fd), ("counts", fc), ("dwell", fw)):
            worst[k] = max(worst.get(k, 0.0), v)
        assert max(fp, fd, fc, fw) <= 1.0, (a.matrix, fp, fd, fc, fw)
    print(f"substmap whole tree S={states}: device against oracle, worst fractions of the summed bounds {worst}")


@pytest.mark.gpu
def test_refusals(product):
    L = product.lib
    INVALID = 113                                          # PLL_ERROR_PARAM_INVALID

    def refused(call):
        product.errno = 0
        with pytest.raises(RuntimeError):
            call()
        assert product.errno == INVALID, product.errmsg

    with build_case(product, 4, 4, 33, True) as inst:
        t = inst.tree
        edge = (t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix)
        product.errno = 0
        assert not L.pllhip_substmap_edge(None, *edge, inst.params_p, 0) and product.errno == INVALID
        product.errno = 0
        assert not L.pllhip_substmap_edge(inst.p, *edge, None, 0) and product.errno == INVALID
        refused(lambda: pc.EdgePairs.edge(inst, 99, *edge[1:]))
        refused(lambda: pc.EdgePairs.edge(inst, edge[0], 99, *edge[2:]))
        refused(lambda: pc.EdgePairs.edge(inst, *edge[:2], 99, *edge[3:]))
        refused(lambda: pc.EdgePairs.edge(inst, *edge[:4], 99))
        refused(lambda: pc.EdgePairs.edge(inst, *edge, params=[0, 0, 7, 0]))
        refused(lambda: pc.EdgePairs.edge(inst, *edge, flags=2))
        L.pllhip_edge_pairs_destroy(None)
        with pc.EdgePairs.edge(inst, *edge) as ok:                     # ... and the partition still serves
            assert ok.differ is None and ok.F.shape == (4, 4, 4)
    with build_case(product, 4, 4, 33, True, attributes=pc.PLL_ATTRIB_AB_FLAG | pc.PLL_ATTRIB_AB_LEWIS) as asc:
        asc.set_asc(pc.PLL_ATTRIB_AB_LEWIS)
        pc.full_traversal(asc)
        t = asc.tree
        with pc.EdgePairs.edge(asc, t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix,
                               WITH_SITES) as ep:                     # allowed: the expectations of the observed sites
            assert ep.sites == 33 and ep.differ.shape == (33,)


@pytest.mark.gpu
def test_a_partition_on_two_shards_is_refused(product):
    L = product.lib
    if L.pllhip_device_count() < 2:
        pytest.skip("one device visible: no partition can be spread over two")
    assert L.pllhip_set_sharding(2, None)
    try:
        shard = build_case(product, 20, 4, 161, True)
    finally:
        assert L.pllhip_set_sharding(0, None)
    with shard:
        t = shard.tree
        product.errno = 0
        with pytest.raises(RuntimeError):
            pc.EdgePairs.edge(shard, t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix)
        assert product.errno == 113
