"""The numpy restatements behind the distance and neighbour-joining tests (tests/nj_reference.py,
tests/distance_reference.py), checked on the CPU, and the symbols of the interface."""
import numpy as np
import pytest

import distance_reference as dr
import nj_reference as njr
import pllhip_ctypes as pc

NEW_NAMES = """pllhip_distances_partition pllhip_distances_msa pllhip_distmat_from_host pllhip_distmat_destroy
pllhip_distmat_size pllhip_distmat_get pllhip_distmat_compared pllhip_distmat_counts pllhip_distmat_no_overlap
pllhip_distmat_nj pllhip_distmat_nj_joins pllhip_distances_last_times""".split()


def test_symbols_are_exported(product_nogpu):
    missing = [n for n in NEW_NAMES if n not in pc.PLLHIP_H_FUNCTIONS or not hasattr(product_nogpu.lib, n)]
    assert not missing, missing


# ---------------------------------------------------------------------------------------------------------------------
# neighbour joining
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4, 5, 7, 64, 65, 257])
def test_nj_recovers_additive_trees(T):
    rng = np.random.default_rng(400 + T)
    dist, splits = njr.random_tree(T, rng)
    slots, lengths = njr.nj(dist)
    assert len(slots) == len(lengths) == 2 * (T - 3) + 3
    assert njr.splits_of_joins(T, slots) == splits
    # an additive matrix gives its own branch lengths back, up to rounding
    assert lengths.min() > 0.05 - 1e-9 and lengths.max() < 0.3 + 1e-9


def test_nj_ties_go_to_the_smallest_pair():
    d = np.ones((9, 9)) - np.eye(9)
    slots, lengths = njr.nj(d)
    assert (slots[0], slots[1]) == (0, 1)
    assert list(slots[-3:]) == sorted(slots[-3:])
    assert len(njr.splits_of_joins(9, slots)) == 9 + 6


def test_nj_three_taxa_is_the_star():
    d = np.array([[0, 0.3, 0.5], [0.3, 0, 0.6], [0.5, 0.6, 0]])
    slots, lengths = njr.nj(d)
    assert list(slots) == [0, 1, 2]
    assert np.allclose(lengths, [0.1, 0.2, 0.4])


# ---------------------------------------------------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------------------------------------------------
def test_counts_are_symmetric_and_add_up_to_the_compared_sites():
    rng = np.random.default_rng(5)
    S, T, L = 4, 7, 300
    codes = rng.integers(0, S, size=(T, L)).astype(np.uint8)
    codes[rng.uniform(size=codes.shape) < 0.2] = dr.NONE
    codes[3] = dr.NONE
    codes[5] = codes[1]
    w = rng.integers(1, 300, size=L)
    N = dr.counts(codes, w, S)
    assert np.array_equal(N, N.transpose(1, 0, 3, 2))
    assert np.array_equal(N.sum(axis=(2, 3)), dr.compared(codes, w))
    assert N[3].sum() == 0 and np.array_equal(N[1, 5], np.diag(np.diag(N[1, 1])))
    p = dr.p_matrix(N)
    assert p[1, 5] == 0.0 and p[3, 0] == 10.0 and np.array_equal(p, p.T)


def test_codes_of_masks():
    cmap = [0] * 256
    for k, c in enumerate(b"ACGT"):
        cmap[c] = 1 << k
    cmap[ord("-")] = 15
    cmap[ord("R")] = 5
    rows = np.frombuffer(b"ACGT-R", dtype=np.uint8)[None, :]
    assert list(dr.codes_of_rows(rows, cmap, 4)[0]) == [0, 1, 2, 3, dr.NONE, dr.NONE]


# ---------------------------------------------------------------------------------------------------------------------
# the ML distance
# ---------------------------------------------------------------------------------------------------------------------
def model_instance(lib, S, R, subst, freqs, alpha, pinv):
    inst = pc.Instance(lib, 3, S, 8, R, attributes=0, scalers=False, clv_buffers=1, prob_matrices=1)
    rates = lib.gamma_cats(alpha, R) if R > 1 else np.ones(1)
    inst.set_model(subst, freqs, rates)
    if pinv > 0:
        inst.set_pinv(pinv)
    assert inst.L.pll_update_eigen(inst.p, 0)
    return inst


@pytest.mark.parametrize("S, R, pinv", [(4, 4, 0.0), (4, 4, 0.2), (20, 4, 0.0)])
def test_reference_pmatrix_is_the_oracles(oracle, S, R, pinv):
    if S == 4:
        subst, freqs = pc.DNA_GTR_RATES, pc.DNA_FREQS
    else:
        subst, freqs = pc.protein_model()
    with model_instance(oracle, S, R, subst, freqs, 0.7, pinv) as inst:
        model = dr.Model(inst)
        for t in (1e-6, 0.013, 0.4, 3.0):
            inst.update_pmatrices([0], [t])
            want = inst.get_pmatrix(0)
            for r in range(R):
                got = model.pmatrix(t, r).astype(np.float64)
                assert np.max(np.abs(got - want[r])) < 1e-12, (t, r)


def test_ml_distance_is_the_jc_formula_under_the_jc_model(oracle):
    rng = np.random.default_rng(6)
    S, L = 4, 500
    base = rng.integers(0, S, size=L)
    codes = np.stack([base] + [np.where(rng.uniform(size=L) < share, (base + rng.integers(1, S, size=L)) % S, base)
                               for share in (0.05, 0.2, 0.45)]).astype(np.uint8)
    N = dr.counts(codes, None, S)
    jc = dr.jc_matrix(N, S)
    with model_instance(oracle, S, 1, np.ones(6), np.full(4, 0.25), 1.0, 0.0) as inst:
        model = dr.Model(inst)
        for i in range(4):
            for j in range(i + 1, 4):
                d = dr.ml_distance(model, N[i, j])
                assert abs(d - jc[i, j]) <= 1e-12, (i, j, d, jc[i, j])
        assert dr.ml_distance(model, N[0, 0]) == 1e-6                      # identical: the lower bound
        assert dr.ml_distance(model, np.ones((4, 4), dtype=np.int64) - np.eye(4, dtype=np.int64)) == 10.0
