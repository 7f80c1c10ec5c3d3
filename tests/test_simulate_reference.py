"""Simulated alignments on the CPU: the numpy reference (tests/simulate_reference.py) against theory with the
oracle's matrices and per-site likelihoods, the edge cases of `pick`, and the host plan (pll-modules_amd/csrc/
sim_plan.cpp) through tests/sim_plan_host_check.cpp, a program of its own built with -fsanitize=address,undefined.

The statistical tests state a condition, not a measurement: every cell with expectation >= 100 has
|count - n p| <= 6 sqrt(n p (1 - p)).  Under the normal approximation a cell fails with probability 2e-9; with at most
257 cells a correct sampler fails with probability < 1e-6.  The seed (simulate_reference.STAT_SEED) was fixed after
the reference had been seen to pass with it."""
import os
import subprocess

import numpy as np
import pytest

import pllhip_ctypes as pc
import simulate_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_setup(oracle, tips):
    """DNA, GTR + G4 + I on a random tree, the oracle's matrices: (inst, edges, pmats)"""
    inst = pc.build_instance(oracle, 4, 4, tips, 8, pinv=sr.STAT_PINV, tree=pc.Tree(tips, 52, 53))
    t = inst.tree
    inst.update_pmatrices(np.arange(t.nedges), t.brlens)
    pmats = {m: inst.get_pmatrix(m) for m in range(t.nedges)}
    edges = list(zip(*[a.tolist() for a in pc.tree_edges(t)]))
    return inst, edges, pmats


def tip_path(tree, a, b):
    """matrix indices of the edges between tips a and b"""
    stack = [(a, -1, [])]
    while stack:
        node, came, path = stack.pop()
        if node == b:
            return path
        for v, k in tree.adj[node]:
            if v != came:
                stack.append((v, node, path + [k]))
    raise AssertionError("no path")


@pytest.mark.parametrize("tips,pair", [(3, (0, 2)), (5, (1, 4))])
def test_joint_counts_of_two_tips_match_theory(oracle, tips, pair):
    """n * sum_c w_c [(1 - p) pi_i P_ij(path) + p pi_i delta_ij] against the 4 x 4 counts of two tips"""
    inst, edges, pmats = oracle_setup(oracle, tips)
    with inst:
        weights, pinv, freqs = sr.model_arrays(inst)
        n = sr.STAT_SITES
        rows = sr.simulate(sr.STAT_SEED, n, 1, weights, pinv, freqs, pmats, tips, edges, tips, 2 * tips - 2)[0]
        a, b = pair
        counts = np.bincount(rows[a].astype(np.int64) * 4 + rows[b], minlength=16).reshape(4, 4)
        expected = np.zeros((4, 4))
        for c in range(inst.R):
            P = np.eye(4)
            for m in tip_path(inst.tree, a, b):
                P = P @ pmats[m][c]
            expected += weights[c] * ((1.0 - pinv[c]) * freqs[c][:, None] * P + pinv[c] * np.diag(freqs[c]))
        assert abs(expected.sum() - 1.0) < 1e-9
        assert sr.accept(counts, n * expected) == []


def test_pattern_counts_match_the_oracles_site_likelihoods(oracle):
    """4 tips: the counts of the 256 column patterns against n exp(persite lnL) of a partition whose sites are the
    patterns, same model and tree"""
    with sr.pattern_instance(oracle, pc) as inst:
        t = inst.tree
        pc.full_traversal(inst)
        sa, sb = t.scaler_of(t.root_a), t.scaler_of(t.root_b)
        _, persite = inst.edge_lnl(t.root_a, sa, t.root_b, sb, t.root_matrix, persite=True)
        prob = np.exp(persite)
        assert abs(prob.sum() - 1.0) < 1e-9
        pmats = {m: inst.get_pmatrix(m) for m in range(t.nedges)}
        edges = list(zip(*[a.tolist() for a in pc.tree_edges(t)]))
        weights, pinv, freqs = sr.model_arrays(inst)
        n = sr.STAT_SITES
        rows = sr.simulate(sr.STAT_SEED, n, 1, weights, pinv, freqs, pmats, 4, edges, 4, 6)[0]
        assert sr.accept(sr.pattern_counts(rows), n * prob) == []


def test_the_condition_rejects_a_wrong_sampler():
    """the acceptance condition has teeth: counts drawn with one probability 5 % too large (13 sigma of its cell) are refused"""
    rng = np.random.default_rng(5)
    p = np.full(16, 1.0 / 16)
    q = p.copy()
    q[3] *= 1.05
    q /= q.sum()
    n = sr.STAT_SITES
    assert sr.accept(rng.multinomial(n, p), n * p) == []
    assert sr.accept(rng.multinomial(n, q), n * p) != []


def test_pick_edge_cases():
    # u beyond a last sum below 1: the last state, never n
    cum = sr.cumulate([0.25, 0.25, 0.25, 0.2499999])
    assert cum[-1] < 1.0
    assert sr.pick(np.array(0.99999999), cum) == 3 and sr.pick_bisect(0.99999999, cum) == 3
    assert sr.pick(np.array(np.nextafter(1.0, 0.0)), cum) == 3
    # a last sum above 1 changes nothing either
    assert sr.pick(np.array(0.9999), sr.cumulate([0.5, 0.3, 0.3])) == 2
    # zero-probability states are never drawn
    cum = sr.cumulate([0.0, 0.5, 0.0, 0.0, 0.5, 0.0])
    u = sr.uniform(1, 0, 0, np.arange(100000, dtype=np.uint64))
    drawn = sr.pick(u, cum[None, :])
    assert set(np.unique(drawn)) == {1, 4}
    assert sr.pick(np.array(0.0), cum) == 1 and sr.pick(np.array(0.5), cum) == 4
    # a negative round-off entry counts as 0: the sums stay monotone and the state is not drawn
    cum = sr.cumulate([0.3, -1e-17, 0.7])
    assert np.array_equal(cum, [0.3, 0.3, 1.0])
    assert set(np.unique(sr.pick(u, cum[None, :]))) == {0, 2}
    assert sr.pick(np.array(0.3), cum) == 2
    # u is in [0, 1)
    assert u.min() >= 0.0 and u.max() < 1.0


def test_bisection_agrees_with_the_counting_definition():
    rng = np.random.default_rng(11)
    rows = 100000
    for n in (2, 4, 20, 61):
        x = rng.random((rows, n))
        x[rng.random((rows, n)) < 0.2] = 0.0                      # zero-probability states
        x[rng.random((rows, n)) < 0.02] *= -1e-12                 # round-off below 0
        x /= np.maximum(x.sum(axis=1, keepdims=True), 1e-300)
        cum = sr.cumulate(x)
        assert (np.diff(cum, axis=1) >= 0).all()
        u = rng.random(rows)
        u[:100] = cum[:100, n // 2]                               # ties: cum[s] <= u counts
        u = np.minimum(u, np.nextafter(1.0, 0.0))
        counted = sr.pick(u, cum)
        bisected = np.array([sr.pick_bisect(u[i], cum[i]) for i in range(rows)])
        assert np.array_equal(counted, bisected)
        assert counted.max() <= n - 1


def test_plan_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "pll-modules_amd", "csrc")
    exe = str(tmp_path / "sim_plan_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-static-libasan", "-static-libubsan",
           "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "sim_plan_host_check.cpp"),
           os.path.join(csrc, "sim_plan.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok")


def test_plan_is_host_only():
    """the planner's boundary: standard headers and its own, so that the check above builds it without HIP"""
    csrc = os.path.join(ROOT, "pll-modules_amd", "csrc")
    for name in ("sim_plan.hpp", "sim_plan.cpp"):
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
        assert all(i.startswith("<") or i == '"sim_plan.hpp"' for i in includes), (name, includes)
        for word in ("Engine", "hip/", "getenv"):
            assert word not in text, (name, word)
