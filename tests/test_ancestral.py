"""Marginal ancestral states for the whole tree: pllhip_node_ancestral_batch (include/pllhip.h) and the driver's
pllhip_eval_compute_ancestral (include/pllhip_eval.h), the counterpart of pllmod_treeinfo_compute_ancestral
(src/tree/treeinfo.c:1611-1718).  CPU tests run the driver on the oracle (per-node pll_compute_node_ancestral and
a host summary); GPU tests run the same driver on the HIP engine (device batch) and compare.

Tolerances are those of tests/test_gpu_parity.py::test_node_ancestral_states: rtol 1e-9, atol 1e-12 up to 20
states, atol 2e-6 at 61."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import pllhip_ctypes as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = pc.PLLHIP_ANC_PROBS
GAP = np.uint8((ord("-") - 48) % 256)         # codes + 48 are the sequence bytes (pc.state_charmap): this one is '-'


def atol_for(states):
    return 1e-12 if states <= 20 else 2e-6


# ---------------------------------------------------------------------------
# the two-partition build of tests/test_eval_driver.py (same seeds), with the knobs these tests turn
# ---------------------------------------------------------------------------
def build(lib, ntips=14, sizes=(400, 150), attributes=0, uniform_dna=False, gap_column=None, remote=()):
    t = pc.Tree(ntips, 42, 43)
    ev = pc.Evaluation(lib, t.newick(), nparts=2)
    dna = pc.random_codes(ntips, sizes[0], 4)
    prot = pc.random_codes(ntips, sizes[1], 20, seed=99)
    if gap_column is not None:
        dna[:, gap_column] = GAP
    r, f = pc.protein_model()
    if 0 in remote:
        ev.add_remote_partition(0)
    else:
        ev.add_partition(0, 4, sizes[0], 4, dna, pc.DNA_GTR_RATES, [0.25] * 4 if uniform_dna else pc.DNA_FREQS, 0.7,
                         attributes=attributes)
    if 1 in remote:
        ev.add_remote_partition(1)
    else:
        ev.add_partition(1, 20, sizes[1], 4, prot, r, f, 0.5, attributes=attributes)
    ev.pytree = t
    return ev


def addr(ptr):
    return C.addressof(ptr.contents)


def python_postorder(ev):
    """inner records in a full post-order from the tree's vroot, written from the definition of pll_utree_traverse:
    the subtree behind root->back first, then root; below a record, the subtrees behind next->back, next->next->back"""
    out = []

    def walk(rec):
        if rec.contents.next:
            s = rec.contents.next
            while addr(s) != addr(rec):
                walk(s.contents.back)
                s = s.contents.next
            out.append(rec)

    vroot = ev.utree.contents.vroot
    walk(vroot.contents.back)
    walk(vroot)
    return out


def per_node_tables(ev, records):
    """what the reference's loop computes: root at the record, incremental evaluation, pll_compute_node_ancestral
    per partition; [node][partition] -> sites x states"""
    L = ev.L
    old = L.pllhip_eval_root(ev.ev)
    out = []
    for rec in records:
        assert L.pllhip_eval_set_root(ev.ev, rec)
        ev.loglh(True)
        n, b = rec.contents, rec.contents.back.contents
        out.append([inst.node_ancestral(n.clv_index, n.scaler_index, b.clv_index, b.scaler_index, n.pmatrix_index)
                    for inst in ev.parts])
    assert L.pllhip_eval_set_root(ev.ev, old)
    return out


def check_summary(anc, states_of):
    """states == argmax(probs) with the first index on ties, state_probs == max, exactly"""
    for k, S in enumerate(states_of):
        for i in range(len(anc.node_clv)):
            rows = anc.rows(i, k, S)
            a, b = anc.site_offset[k], anc.site_offset[k + 1]
            assert np.array_equal(anc.states[i, a:b], np.argmax(rows, axis=1).astype(np.uint8))
            assert np.array_equal(anc.state_probs[i, a:b], rows.max(axis=1))


# ---------------------------------------------------------------------------
# CPU: the driver on the oracle
# ---------------------------------------------------------------------------
def test_brute_force_posteriors(oracle):
    """5 tips, 4 states, 2 rate categories, 3 sites, coded tips with a partial ambiguity code ('R' = A or G) and a
    gap: every inner node's posterior from all 4^3 assignments of the inner states, with the oracle's P-matrices"""
    ntips, S, R = 5, 4, 2
    seqs = ["0R2", "12-", "301", "0R3", "210"]
    t = pc.Tree(ntips, 7, 8)
    with pc.Evaluation(oracle, t.newick(), nparts=1) as ev:
        inst = pc.Instance(oracle, ntips, S, 3, R, attributes=pc.PLL_ATTRIB_PATTERN_TIP)
        inst.set_model(pc.DNA_GTR_RATES, pc.DNA_FREQS, oracle.gamma_cats(0.7, R))
        cmap = pc.state_charmap(S)
        cmap[ord("R")] = np.uint64(0b0101)
        for k in range(ntips):
            inst.set_tip_states(ev.tip_clv[k], cmap, seqs[k].encode())
        assert ev.L.pllhip_eval_set_partition(ev.ev, 0, inst.p, inst.params_p)
        ev.parts.append(inst)
        ev.loglh()
        anc = ev.compute_ancestral(PROBS)

        # the tree as the library holds it: edges (clv, clv, pmatrix), tips by clv index
        edges = {}
        for rec in ev.records():
            n, b = rec.contents, rec.contents.back.contents
            edges[n.pmatrix_index] = (n.clv_index, b.clv_index)
        tip_seq = {ev.tip_clv[k]: seqs[k] for k in range(ntips)}
        inner = sorted({c for e in edges.values() for c in e if c not in tip_seq})
        assert len(inner) == 3 and len(edges) == 7
        P = {m: inst.get_pmatrix(m) for m in edges}
        pi, w = np.array(pc.DNA_FREQS), np.full(R, 1.0 / R)
        # orient the inner edges away from inner[0] (reversibility: the joint probability does not depend on the root)
        adj = {u: [] for u in inner}
        for m, (a, b) in edges.items():
            for x, y in ((a, b), (b, a)):
                if x in adj:
                    adj[x].append((y, m))
        order, seen = [], {inner[0]}
        stack = [inner[0]]
        while stack:
            u = stack.pop()
            for v, m in adj[u]:
                if v in tip_seq:
                    order.append((u, v, m))
                elif v not in seen:
                    seen.add(v)
                    order.append((u, v, m))
                    stack.append(v)
        want = np.zeros((3, 3, S))            # [inner node][site][state]
        for site in range(3):
            masks = {c: int(cmap[ord(s[site])]) for c, s in tip_seq.items()}
            for r in range(R):
                for assign in itertools.product(range(S), repeat=3):
                    x = dict(zip(inner, assign))
                    joint = pi[x[inner[0]]]
                    for u, v, m in order:
                        if v in tip_seq:
                            joint *= sum(P[m][r, x[u], j] for j in range(S) if (masks[v] >> j) & 1)
                        else:
                            joint *= P[m][r, x[u], x[v]]
                    for k, u in enumerate(inner):
                        want[k, site, x[u]] += w[r] * joint
        want /= want.sum(axis=2, keepdims=True)
        assert sorted(anc.node_clv.tolist()) == inner
        for i, clv in enumerate(anc.node_clv):
            got = anc.rows(i, 0, S)
            assert np.allclose(got.sum(axis=1), 1.0, atol=1e-12)
            assert np.allclose(got, want[inner.index(int(clv))], rtol=0, atol=1e-12)
        check_summary(anc, [S])


def test_driver_contract_on_oracle(oracle):
    with build(oracle) as ev:
        before = ev.loglh()
        root0 = addr(ev.L.pllhip_eval_root(ev.ev))
        anc = ev.compute_ancestral(PROBS)
        # the root is restored, and nothing the evaluator knows was damaged
        assert addr(ev.L.pllhip_eval_root(ev.ev)) == root0
        assert abs(ev.loglh(True) - before) <= 1e-8 * abs(before)
        # node order: an independent post-order from vroot
        recs = python_postorder(ev)
        assert len(recs) == ev.ntips - 2 == len(anc.node_clv)
        assert [r.contents.node_index for r in recs] == anc.node_index.tolist()
        assert anc.partition_indices.tolist() == [0, 1]
        assert anc.site_offset.tolist() == [0, 400, 550] and anc.prob_offset.tolist() == [0, 1600, 1600 + 150 * 20]
        # probs: bit for bit what per-node calls on the same library return after the same re-rooting
        tables = per_node_tables(ev, recs)
        for i in range(len(recs)):
            for k, S in enumerate((4, 20)):
                assert np.array_equal(anc.rows(i, k, S), tables[i][k])
        check_summary(anc, [4, 20])
        # without the flag: no table, the same summary
        short = ev.compute_ancestral(0)
        assert short.probs is None
        assert np.array_equal(short.states, anc.states) and np.array_equal(short.state_probs, anc.state_probs)
        assert addr(ev.L.pllhip_eval_root(ev.ev)) == root0
        assert abs(ev.loglh(True) - before) <= 1e-8 * abs(before)


def test_tie_rule_on_an_all_gap_column(oracle):
    """uniform frequencies and a column of gaps: the states of such a row are equal up to the rounding of the
    P-matrices' row sums, and where two of them are the same double the first index has to win: the oracle's rows
    of this column hold an exact tie for the maximum at all 12 nodes."""
    col = 17
    with build(oracle, uniform_dna=True, gap_column=col) as ev:
        ev.loglh()
        anc = ev.compute_ancestral(PROBS)
        check_summary(anc, [4, 20])
        ties = 0
        for i in range(len(anc.node_clv)):
            row = anc.rows(i, 0, 4)[col]
            assert np.allclose(row, 0.25, rtol=0, atol=1e-12)
            ties += int((row == row.max()).sum() > 1)
            assert anc.states[i, col] == int(np.argmax(row)) and anc.state_probs[i, col] == row.max()
        print(f"all-gap column: {ties} of {len(anc.node_clv)} nodes hold an exact tie for the maximum")
        assert ties > 0                 # (12 of 12 on the oracle as built by oracle/Makefile)


def test_remote_partition_is_skipped(oracle):
    with build(oracle) as whole, build(oracle, remote=(1,)) as part:
        whole.loglh()
        part.loglh()
        a, b = whole.compute_ancestral(PROBS), part.compute_ancestral(PROBS)
        assert b.partition_indices.tolist() == [0]
        assert b.site_offset.tolist() == [0, 400] and b.prob_offset.tolist() == [0, 1600]
        assert np.array_equal(b.probs, a.probs[:, :1600])
        assert np.array_equal(b.states, a.states[:, :400]) and np.array_equal(b.state_probs, a.state_probs[:, :400])


def test_oracle_excludes_no_row_at_the_gpu_shape(oracle):
    """the shape of the GPU test below: how many rows have their two largest probabilities within 1e-9"""
    with build(oracle, sizes=(77, 33)) as ev:
        ev.loglh()
        anc = ev.compute_ancestral(PROBS)
        assert close_rows(anc, (4, 20)) == 0


def close_rows(anc, states_of):
    n = 0
    for k, S in enumerate(states_of):
        for i in range(len(anc.node_clv)):
            top = np.sort(anc.rows(i, k, S), axis=1)
            n += int((top[:, -1] - top[:, -2] <= 1e-9).sum())
    return n


def test_host_code_under_sanitizers(tmp_path):
    """tests/ancestral_host_check.c: the new driver code on the oracle's sources (a 6-tip tree, both flag settings,
    the error path with a partition whose rate matrix is degenerate), built with -fsanitize=address,undefined as a program
    of its own and run here on the CPU"""
    host = os.path.join(ROOT, "pll-modules_amd", "csrc", "host")
    srcs = [os.path.join(ROOT, "oracle", f) for f in ("orc_partition.c", "orc_model.c", "orc_kernels.c")] + \
           [os.path.join(host, f) for f in ("pll_utree.c", "pll_notimpl.c", "pll_random.c", "pll_maps.c",
                                            "pll_utree_moves.c", "pllhip_eval.c", "pllhip_search.c", "pll_repeats.c")]
    exe = str(tmp_path / "ancestral_host_check")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"),
           "-o", exe, os.path.join(ROOT, "tests", "ancestral_host_check.c")] + srcs + ["-lm"]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok")


# ---------------------------------------------------------------------------
# GPU: the batch call against the oracle's per-node call
# ---------------------------------------------------------------------------
PARITY_SHAPES = [(4, 4), (20, 4), (5, 4), (10, 4), (16, 4), (2, 4), (61, 4), (4, 3), (20, 1)]
PARITY_SITES = [1, 33, 77, 2085]     # a partial block, a block plus a site, the per-node test's size, > 1 workgroup + tail


@pytest.mark.gpu
@pytest.mark.parametrize("coded", [True, False], ids=["coded", "tip-vectors"])
@pytest.mark.parametrize("states,rate_cats", PARITY_SHAPES)
def test_batch_against_oracle_per_node(product, oracle, states, rate_cats, coded):
    """the root edge's triple and the reversed one in one batch (count = 2).  The root edge of pc.Tree ends in a
    tip: `other` is a tip (codes, or a tip vector with coded=False) in the first entry, `node` is in the second."""
    for nsites in PARITY_SITES:
        a = pc.build_instance(product, states=states, rate_cats=rate_cats, ntips=7, nsites=nsites, coded=coded)
        b = pc.build_instance(oracle, states=states, rate_cats=rate_cats, ntips=7, nsites=nsites, coded=coded,
                              tree=a.tree)
        with a, b:
            pc.full_traversal(a)
            pc.full_traversal(b)
            t = a.tree
            assert t.root_b < t.ntips
            nodes, others, mats = [t.root_a, t.root_b], [t.root_b, t.root_a], [t.root_matrix] * 2
            st, sp, pr, intact = a.node_ancestral_batch(nodes, others, mats, PROBS, pad=8)
            assert intact                                   # no byte in front of or behind `sites` elements
            st0, sp0, none, intact0 = a.node_ancestral_batch(nodes, others, mats, 0, pad=8)
            assert intact0 and none is None
            assert np.array_equal(st0, st) and np.array_equal(sp0, sp)
            for k in range(2):
                want = b.node_ancestral(nodes[k], t.scaler_of(nodes[k]), others[k], t.scaler_of(others[k]), mats[k])
                err = float(np.max(np.abs(pr[k] - want)))
                print(f"S={states} R={rate_cats} N={nsites} coded={coded} entry {k}: max |diff| {err:.3g}")
                assert np.allclose(pr[k].sum(axis=1), 1.0, atol=1e-12)
                assert np.allclose(pr[k], want, rtol=1e-9, atol=atol_for(states))
                assert np.array_equal(st[k], np.argmax(pr[k], axis=1).astype(np.uint8))
                assert np.array_equal(sp[k], pr[k].max(axis=1))


# ---------------------------------------------------------------------------
# GPU: the driver on the product against the driver on the oracle
# ---------------------------------------------------------------------------
GPU_SIZES = (77, 33)
_cache = {}


def oracle_run(oracle, sizes):
    """the oracle's result for a shape, computed once and shared (never modified)"""
    if sizes not in _cache:
        with build(oracle, sizes=sizes) as ev:
            ev.loglh()
            _cache[sizes] = ev.compute_ancestral(PROBS)
    return _cache[sizes]


def product_run(product, sizes, attributes=0, transient=False, shard_second=False, flags=PROBS):
    L = product.lib
    t = pc.Tree(14, 42, 43)
    ev = pc.Evaluation(product, t.newick(), nparts=2)
    try:
        r, f = pc.protein_model()
        ev.add_partition(0, 4, sizes[0], 4, pc.random_codes(14, sizes[0], 4), pc.DNA_GTR_RATES, pc.DNA_FREQS, 0.7,
                         attributes=attributes)
        if shard_second:
            assert L.pllhip_set_sharding(2, None)
        try:
            ev.add_partition(1, 20, sizes[1], 4, pc.random_codes(14, sizes[1], 20, seed=99), r, f, 0.5,
                             attributes=attributes)
        finally:
            assert L.pllhip_set_sharding(0, None)
        if shard_second:
            assert L.pllhip_shard_count(ev.parts[1].p) == 2
        if transient:
            ev.set_transient(1)
        ev.loglh()
        return ev.compute_ancestral(flags)
    finally:
        ev.close()


def same_bits(a, b):
    return (np.array_equal(a.states, b.states) and np.array_equal(a.state_probs, b.state_probs) and
            np.array_equal(a.probs, b.probs) and np.array_equal(a.node_index, b.node_index))


def check_against_oracle(got, want, states_of=(4, 20)):
    assert np.array_equal(got.node_index, want.node_index)
    assert np.array_equal(got.site_offset, want.site_offset) and np.array_equal(got.prob_offset, want.prob_offset)
    rows = excluded = 0
    for k, S in enumerate(states_of):
        a, b = want.site_offset[k], want.site_offset[k + 1]
        for i in range(len(want.node_clv)):
            g, w = got.rows(i, k, S), want.rows(i, k, S)
            assert np.allclose(g, w, rtol=1e-9, atol=atol_for(S))
            top = np.sort(w, axis=1)
            clear = top[:, -1] - top[:, -2] > 1e-9
            rows += len(clear)
            excluded += int((~clear).sum())
            assert np.array_equal(got.states[i, a:b][clear], want.states[i, a:b][clear])
            assert np.allclose(got.state_probs[i, a:b], want.state_probs[i, a:b], rtol=1e-9, atol=atol_for(S))
    assert excluded * 100 <= rows, (excluded, rows)
    check_summary(got, states_of)


@pytest.mark.gpu
def test_driver_on_gpu_against_driver_on_oracle(product, oracle):
    """14 tips, DNA 77 + protein 33 sites.  States are compared wherever the oracle's two largest probabilities of
    the row differ by more than 1e-9; on the oracle alone that rule excludes 0 of the 12 x 110 rows of this shape
    (test_oracle_excludes_no_row_at_the_gpu_shape), the cap here is 1 %.
    Site repeats and evaluate-only traversals before the call give the bits of the plain run.
    A partition of 33 sites cannot be spread over two devices (the engine keeps fewer than 64 sites per device on
    one), so the sharded variant runs the same build with 161 protein sites -- two shards, 96 + 65 sites -- against
    the oracle and against its own plain run."""
    want = oracle_run(oracle, GPU_SIZES)
    plain = product_run(product, GPU_SIZES)
    check_against_oracle(plain, want)
    short = product_run(product, GPU_SIZES, flags=0)
    assert short.probs is None
    assert np.array_equal(short.states, plain.states) and np.array_equal(short.state_probs, plain.state_probs)
    assert same_bits(product_run(product, GPU_SIZES, attributes=pc.PLL_ATTRIB_SITE_REPEATS), plain)
    assert same_bits(product_run(product, GPU_SIZES, transient=True), plain)
    wide = (77, 161)
    plain_wide = product_run(product, wide)
    check_against_oracle(plain_wide, oracle_run(oracle, wide))
    assert same_bits(product_run(product, wide, shard_second=True), plain_wide)


@pytest.mark.gpu
def test_results_do_not_depend_on_chunking_or_run_order(product, monkeypatch):
    """the two-partition build with 77 sites in the 20-state partition (and 33 DNA sites) through the driver: a
    staging budget of one entry per chunk against the default, each twice; all four bit-identical"""
    runs = []
    for budget in ("1", None, "1", None):
        if budget is None:
            monkeypatch.delenv("PLLHIP_ANC_STAGING_BYTES", raising=False)
        else:
            monkeypatch.setenv("PLLHIP_ANC_STAGING_BYTES", budget)
        runs.append(product_run(product, (33, 77)))
        chunks = C.c_ulonglong(0)
        product.lib.pllhip_node_ancestral_last_times(None, C.byref(chunks))
        # (the last batch is the protein partition's: 12 nodes, one per chunk, or all in one)
        assert chunks.value == (12 if budget else 1)
    for other in runs[1:]:
        assert same_bits(other, runs[0])


@pytest.mark.gpu
def test_batch_against_the_per_node_call_on_the_product(product):
    """for every inner node the batch's table agrees with the product's own pll_compute_node_ancestral.  The two
    kernels sum in different orders (matrix-core k-steps against a serial loop), so bit identity is not required:
    the tolerances are those of the parity test."""
    with build(product, sizes=GPU_SIZES) as ev:
        ev.loglh()
        anc = ev.compute_ancestral(PROBS)
        tables = per_node_tables(ev, python_postorder(ev))
        for i in range(len(anc.node_clv)):
            for k, S in enumerate((4, 20)):
                assert np.allclose(anc.rows(i, k, S), tables[i][k], rtol=1e-9, atol=atol_for(S))
