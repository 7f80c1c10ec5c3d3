"""pllhip_empirical_frequencies / _subst_rates / _invariant_sites and pllhip_msa_compute_stats on the device
(csrc/pll_msa_stats_dev.hip) against the exact restatement of tests/test_msa_stats_restatement.py.

Integers and index lists: equal.  Exchangeabilities: bit-equal (the same integers through the same double
operations).  Frequencies from masks: within 2 ulp of the exactly rounded value (the finish is S + 1 long-double terms
and one rounding).  Frequencies from probability vectors: within (tips * sites + 2) * 2^-52 relative, and bit-equal
from call to call."""
import ctypes as C

import numpy as np
import pytest

import pllhip_ctypes as pc
import test_msa_stats_restatement as rs

pytestmark = pytest.mark.gpu

DNA = b"ACGTACGTACGTACGTUacgtRYMKSWBDHVN-?X"
AA = b"ARNDCQEGHILKMFPSTWYVARNDCQEGHILKMFPSTWYVarndcBZX*-?"
BIN = b"01010101-?"
# 61 states: one character per state, a gap and three ambiguous sets of 2, 3 and 31 states
S61_CHARS = bytes(range(48, 48 + 61))
S61 = S61_CHARS + S61_CHARS + b"-!#$"


def s61_map():
    m = [0] * 256
    for k, c in enumerate(S61_CHARS):
        m[c] = 1 << k
    m[ord("-")] = (1 << 61) - 1
    m[ord("!")] = (1 << 3) | (1 << 40)
    m[ord("#")] = (1 << 0) | (1 << 33) | (1 << 60)
    m[ord("$")] = sum(1 << k for k in range(15, 46))
    return m


def alphabet(product, name):
    """(states, character map, characters to draw from)"""
    if name == "s61":
        return 61, s61_map(), S61
    return {"bin": (2, product.char_map("pll_map_bin"), BIN), "nt": (4, product.char_map("pll_map_nt"), DNA),
            "aa": (20, product.char_map("pll_map_aa"), AA)}[name]


def draw(rng, chars, T, L):
    rows = rng.choice(np.frombuffer(chars, dtype=np.uint8), size=(T, L))
    for n in range(2, L, 5):                          # some columns of one unambiguous character
        rows[:, n] = chars[n % 2]
    return np.ascontiguousarray(rows)


def partition(lib, rows, cmap, S, weights=None, attributes=pc.PLL_ATTRIB_PATTERN_TIP, vectors=None, rate_cats=2):
    """a partition whose tips are `rows` (pll_set_tip_states), or `vectors` [T, L, S] (pll_set_tip_clv)"""
    T, L = (len(rows), len(rows[0])) if vectors is None else vectors.shape[:2]
    inst = pc.Instance(lib, T, S, L, rate_cats, attributes=attributes, scalers=False, prob_matrices=1,
                       clv_buffers=max(1, T - 2))
    for t in range(T):
        if vectors is None:
            inst.set_tip_states(t, cmap, bytes(rows[t]))
        else:
            inst.set_tip_clv(t, vectors[t])
    if weights is not None:
        inst.set_pattern_weights(weights)
    return inst


def within_ulps(got, want, ulps=2):
    """(0 / 0 where every character is a gap: NaN in both)"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.all(np.abs(got - want)[~nan] <= ulps * np.spacing(np.abs(want[~nan])))


def check_partition(lib, inst, masks, weights, S, gaps=None):
    w = np.ones(masks.shape[1], dtype=np.uint32) if weights is None else weights
    freqs = lib.empirical_frequencies(inst.p)
    assert freqs is not None, (lib.errno, lib.errmsg)
    want = rs.frequencies(masks, w, S, with_gaps=True)
    assert within_ulps(freqs, want), (freqs, want)
    rates = lib.empirical_subst_rates(inst.p)
    assert rates is not None, (lib.errno, lib.errmsg)
    assert rates.tobytes() == rs.subst_rates(masks, w, S, gaps).tobytes()
    assert lib.empirical_invariant_sites(inst.p) == rs.invariant_partition(masks, w)
    return freqs, rates


def check_alignment(lib, rows, S, cmap, weights=None, mask=pc.MSA_STATS_ALL, labels=None):
    got = lib.msa_compute_stats([bytes(r) for r in rows], S, cmap, weights, mask, labels)
    assert got is not None, (lib.errno, lib.errmsg)
    want = rs.msa_stats([bytes(r) for r in rows], S, cmap, weights, mask, labels)
    for key in ("states", "dup_taxa_pairs", "dup_seqs_pairs", "gap_seqs", "gap_cols", "inv_cols", "gap_prop", "inv_prop"):
        assert got[key] == want[key], (key, got[key], want[key])
    for key in ("freqs", "subst_rates"):
        assert (got[key] is None) == (want[key] is None), key
    if want["freqs"] is not None:
        assert within_ulps(got["freqs"], want["freqs"]), (got["freqs"], want["freqs"])
    if want["subst_rates"] is not None:
        assert got["subst_rates"].tobytes() == want["subst_rates"].tobytes()
    return got


# ---------------------------------------------------------------------------------------------------------------------
# shapes: the 4-sites-per-lane tail, wave and workgroup boundaries, one and many tips, every tier of the state loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 7, 70])
@pytest.mark.parametrize("L", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000])
def test_dna_shapes(product, L, T):
    S, cmap, chars = alphabet(product, "nt")
    rng = np.random.default_rng(1000 * T + L)
    rows = draw(rng, chars, T, L)
    w = rng.integers(1, 1001, size=L).astype(np.uint32)
    check_alignment(product, rows, S, cmap, w)
    masks = rs.masks_of(rows, cmap)
    with partition(product, rows, cmap, S, w) as inst:
        check_partition(product, inst, masks, w, S)


@pytest.mark.parametrize("T", [7, 70])
@pytest.mark.parametrize("name", ["bin", "aa", "s61"])
def test_other_alphabets_1000_sites(product, name, T):
    S, cmap, chars = alphabet(product, name)
    rng = np.random.default_rng(77 + T + S)
    rows = draw(rng, chars, T, 1000)
    w = rng.integers(1, 1001, size=1000).astype(np.uint32)
    check_alignment(product, rows, S, cmap, w)
    masks = rs.masks_of(rows, cmap)
    with partition(product, rows, cmap, S, w) as inst:
        check_partition(product, inst, masks, w, S)


def test_every_character_of_the_maps(product):
    """every character the maps know, ambiguity codes included, one per site and tip"""
    for name in ("bin", "nt", "aa", "s61"):
        S, cmap, _ = alphabet(product, name)
        known = bytes(c for c in range(1, 256) if int(cmap[c]))
        rows = np.stack([np.frombuffer(known, dtype=np.uint8), np.frombuffer(known[::-1], dtype=np.uint8),
                         np.frombuffer(known[1:] + known[:1], dtype=np.uint8)])
        check_alignment(product, rows, S, cmap)
        with partition(product, rows, cmap, S) as inst:
            check_partition(product, inst, rs.masks_of(rows, cmap), None, S)


# ---------------------------------------------------------------------------------------------------------------------
# partition forms
# ---------------------------------------------------------------------------------------------------------------------
FORMS = ["pattern_tip", "states", "clv01", "repeats", "repeats_vectors", "ascertainment", "ascertainment_vectors"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name, T, L", [("nt", 7, 257), ("aa", 7, 257), ("s61", 5, 130), ("bin", 3, 65)])
def test_partition_forms(product, name, T, L, form):
    S, cmap, chars = alphabet(product, name)
    rng = np.random.default_rng(31 + S + len(form))
    rows = draw(rng, chars, T, L)
    w = rng.integers(0, 50, size=L).astype(np.uint32)
    w[0] = 3
    masks = rs.masks_of(rows, cmap)
    attrs = {"pattern_tip": pc.PLL_ATTRIB_PATTERN_TIP, "states": 0, "clv01": 0,
             "repeats": pc.PLL_ATTRIB_PATTERN_TIP | pc.PLL_ATTRIB_SITE_REPEATS, "repeats_vectors": pc.PLL_ATTRIB_SITE_REPEATS,
             "ascertainment": pc.PLL_ATTRIB_PATTERN_TIP | pc.PLL_ATTRIB_AB_FLAG | pc.PLL_ATTRIB_AB_LEWIS,
             "ascertainment_vectors": pc.PLL_ATTRIB_AB_FLAG | pc.PLL_ATTRIB_AB_LEWIS}[form]
    vectors = rs._bits(masks, S).astype(np.float64) if form == "clv01" else None
    with partition(product, rows, cmap, S, w, attributes=attrs, vectors=vectors) as inst:
        if "ascertainment" in form:                     # the extra patterns carry weights of their own: not counted
            inst.set_asc(pc.PLL_ATTRIB_AB_LEWIS, np.full(S, 1000, dtype=np.uint32))
        first = check_partition(product, inst, masks, w, S)
        again = check_partition(product, inst, masks, w, S)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()


def random_vectors(rng, T, L, S):
    """positive vectors, with exact zeros, entries below the 1e-7 of the rates' gap rule, and 0/1 tips among them"""
    v = rng.uniform(0.05, 1.0, size=(T, L, S))
    v[rng.uniform(size=v.shape) < 0.2] = 0.0
    v[rng.uniform(size=v.shape) < 0.05] = 1e-9
    v[:, :, 0] = np.maximum(v[:, :, 0], 0.25)          # no vector is all zero
    v[0] = (v[0] > 0.3).astype(np.float64)
    v[0, :, 0] = 1.0
    v[:, 1, :] = 1.0                                   # a column the rates skip
    return v


@pytest.mark.parametrize("S, T, L, attrs", [(4, 7, 65, 0), (4, 7, 257, 0), (20, 7, 65, 0), (20, 3, 257, pc.PLL_ATTRIB_SITE_REPEATS),
                                            (61, 4, 70, 0), (2, 5, 130, 0)])
def test_probability_vector_tips(product, S, T, L, attrs):
    rng = np.random.default_rng(900 + S + L)
    v = random_vectors(rng, T, L, S)
    w = rng.integers(1, 30, size=L).astype(np.uint32)
    masks, gaps = rs.vector_masks(v)
    with partition(product, None, None, S, w, attributes=attrs, vectors=v) as inst:
        freqs = product.empirical_frequencies(inst.p)
        assert freqs is not None, (product.errno, product.errmsg)
        want = rs.vector_frequencies(v, w)
        bound = (T * L + 2) * 2.0 ** -52
        print("largest relative error", np.max(np.abs(freqs - want) / want), "bound", bound)
        assert np.all(np.abs(freqs - want) <= bound * want), (freqs, want)
        assert product.empirical_frequencies(inst.p).tobytes() == freqs.tobytes()
        rates = product.empirical_subst_rates(inst.p)
        assert rates.tobytes() == rs.subst_rates(masks, w, S, gaps).tobytes()
        assert product.empirical_invariant_sites(inst.p) == rs.invariant_partition(masks, w)


@pytest.mark.parametrize("name, T, L, form", [("nt", 7, 257, "pattern_tip"), ("nt", 7, 257, "states"), ("nt", 7, 257, "vectors"),
                                              ("nt", 70, 1000, "pattern_tip"), ("aa", 7, 1000, "pattern_tip"),
                                              ("aa", 7, 1000, "states"), ("aa", 5, 257, "vectors")])
def test_sharded_partitions(product, name, T, L, form):
    S, cmap, chars = alphabet(product, name)
    rng = np.random.default_rng(55 + T)
    rows = draw(rng, chars, T, L)
    w = rng.integers(1, 1001, size=L).astype(np.uint32)
    dev = (C.c_int * 2)(0, 0)
    assert product.lib.pllhip_set_sharding(2, dev)
    try:
        if form == "vectors":
            v = random_vectors(rng, T, L, S)
            inst = partition(product, None, None, S, w, attributes=0, vectors=v)
        else:
            inst = partition(product, rows, cmap, S, w, attributes=pc.PLL_ATTRIB_PATTERN_TIP if form == "pattern_tip" else 0)
    finally:
        product.lib.pllhip_set_sharding(0, None)
    with inst:
        if product.lib.pllhip_shard_count(inst.p) != 2:
            pytest.skip("pllhip_set_sharding does not put two shards on one device")
        if form == "vectors":
            masks, gaps = rs.vector_masks(v)
            freqs = product.empirical_frequencies(inst.p)
            want = rs.vector_frequencies(v, w)
            assert np.all(np.abs(freqs - want) <= (T * L + 2) * 2.0 ** -52 * want)
            assert product.empirical_frequencies(inst.p).tobytes() == freqs.tobytes()
            assert product.empirical_subst_rates(inst.p).tobytes() == rs.subst_rates(masks, w, S, gaps).tobytes()
        else:
            check_partition(product, inst, rs.masks_of(rows, cmap), w, S)


# ---------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ones", "random", "zeros", "huge"])
def test_weights(product, kind):
    S, cmap, chars = alphabet(product, "nt")
    T, L = 70, 257
    rng = np.random.default_rng(12)
    rows = draw(rng, chars, T, L)
    w = {"ones": np.ones(L, dtype=np.uint32), "random": rng.integers(1, 1001, size=L).astype(np.uint32),
         "zeros": (rng.integers(0, 1001, size=L) * (rng.uniform(size=L) < 0.7)).astype(np.uint32),
         "huge": rng.integers(1, 1001, size=L).astype(np.uint32)}[kind]
    if kind == "huge":                                  # 70^2 * 2^32 * sites stays far below 2^64
        w[[0, 5, 64, 200, 256]] = 2 ** 32 - 1
    w[3] = max(w[3], 1)
    check_alignment(product, rows, S, cmap, w)
    with partition(product, rows, cmap, S, w) as inst:
        check_partition(product, inst, rs.masks_of(rows, cmap), w, S)
    with partition(product, rows, cmap, 4, w, attributes=0) as inst:
        check_partition(product, inst, rs.masks_of(rows, cmap), w, S)


# ---------------------------------------------------------------------------------------------------------------------
# columns built to hit the rules
# ---------------------------------------------------------------------------------------------------------------------
def test_gap_columns_gap_sequences_and_ambiguous_agreement(product):
    S, cmap, _ = alphabet(product, "nt")
    rows = np.stack([np.frombuffer(r, dtype=np.uint8) for r in (
        b"A-RACGTN",
        b"A-MCCGT-",
        b"-----?N-",          # an all-gap sequence
        b"A?WGCGAN",
        b"ANAAC-TC")])
    #     0: A and a gap: invariant in both forms.  1: all gaps: invariant in the partition form only, skipped by the
    #     rates.  2: only ambiguity codes (and A) share A.  3: nothing shared.  7: gaps and one C.
    got = check_alignment(product, rows, S, cmap)
    assert got["gap_cols"] == [1] and got["gap_seqs"] == [2]
    assert got["inv_cols"] == [0, 2, 4, 5, 7]
    masks = rs.masks_of(rows, cmap)
    with partition(product, rows, cmap, S) as inst:
        check_partition(product, inst, masks, None, S)
        assert product.empirical_invariant_sites(inst.p) == 6.0 / 8.0
        inv = np.ctypeslib.as_array(inst.p.contents.invariant, shape=(8,))
        assert list(inv >= 0) == [True, True, True, False, True, True, False, True]
    with partition(product, rows, cmap, S, attributes=0) as inst:
        check_partition(product, inst, masks, None, S)


def test_rate_divisor_fallback_and_both_clamps(product):
    S, cmap, _ = alphabet(product, "nt")
    rng = np.random.default_rng(4)
    rows = rng.choice(np.frombuffer(b"AACCGM-", dtype=np.uint8), size=(70, 300))      # no T: pair[G][T] = 0
    w = rng.integers(1, 10, size=300).astype(np.uint32)
    masks = rs.masks_of(rows, cmap)
    pairs = rs.pair_counts(masks, w, S)
    assert pairs[-1] == 0 and pairs[0] > 50 and pairs[2] == 0
    want = rs.rates_from_pairs(pairs)
    assert want[0] == 50.0 and want[2] == 0.01 and want[-1] == 1.0
    got = check_alignment(product, rows, S, cmap, w, pc.MSA_STATS_SUBST_RATES)
    assert got["subst_rates"].tobytes() == want.tobytes()
    with partition(product, rows, cmap, S, w) as inst:
        check_partition(product, inst, masks, w, S)


# ---------------------------------------------------------------------------------------------------------------------
# alignment form
# ---------------------------------------------------------------------------------------------------------------------
BITS = [pc.MSA_STATS_DUP_TAXA, pc.MSA_STATS_DUP_SEQS, pc.MSA_STATS_GAP_PROP, pc.MSA_STATS_GAP_SEQS, pc.MSA_STATS_GAP_COLS,
        pc.MSA_STATS_INV_PROP, pc.MSA_STATS_INV_COLS, pc.MSA_STATS_FREQS, pc.MSA_STATS_SUBST_RATES, pc.MSA_STATS_ALL]


@pytest.mark.parametrize("mask", BITS)
@pytest.mark.parametrize("weighted", [False, True])
def test_every_mask_bit(product, mask, weighted):
    S, cmap, chars = alphabet(product, "aa")
    rng = np.random.default_rng(8)
    rows = draw(rng, chars, 9, 300)
    rows[4] = rows[1]
    rows[6] = ord("-")
    rows[:, 17] = ord("X")
    labels = [b"t%d" % t for t in range(9)]
    labels[7] = b"t2"
    w = rng.integers(1, 20, size=300).astype(np.uint32) if weighted else None
    got = check_alignment(product, rows, S, cmap, w, mask, labels)
    if mask == pc.MSA_STATS_ALL:
        assert got["dup_seqs_pairs"] == [(1, 4)] and got["dup_taxa_pairs"] == [(2, 7)]
        assert got["gap_seqs"] == [6] and got["gap_cols"] == [17]


def test_unmapped_character(product):
    S, cmap, chars = alphabet(product, "nt")
    rng = np.random.default_rng(9)
    rows = draw(rng, chars, 6, 3000)
    rows[4, 2900] = ord("#")
    rows[2, 17] = ord("!")                       # the first in sequence-major order; rows 0 and 1 are clean
    rows[2, 2000] = ord("#")
    rows[5, 3] = ord("#")
    for mask in (pc.MSA_STATS_ALL, pc.MSA_STATS_FREQS, pc.MSA_STATS_GAP_COLS):
        got = product.msa_compute_stats([bytes(r) for r in rows], S, cmap, None, mask)
        assert got is None
        assert product.errno == rs.PLL_ERROR_MSA_MAP_INVALID
        assert "Unknown state ! at sequence 3 position 18" in product.errmsg, product.errmsg
    with pytest.raises(rs.UnknownState) as e:
        rs.msa_stats([bytes(r) for r in rows], S, cmap)
    assert e.value.args[0] == (3, 18)


# ---------------------------------------------------------------------------------------------------------------------
# consistency with the compression, and the likelihood path
# ---------------------------------------------------------------------------------------------------------------------
def test_consistent_with_pattern_compression(product):
    S, cmap, chars = alphabet(product, "nt")
    rng = np.random.default_rng(10)
    base = draw(rng, chars, 8, 60)
    rows = np.ascontiguousarray(base[:, rng.integers(0, 60, size=1500)])
    full = check_alignment(product, rows, S, cmap, None)
    res = product.compress_site_patterns([r.tobytes() for r in rows], cmap, msa_form=True)
    assert res.ok and res.length < 1500
    small = check_alignment(product, res.rows, S, cmap, res.weights)
    assert within_ulps(small["freqs"], full["freqs"], 4)            # each within 2 ulp of the same exact value
    assert small["gap_prop"] == full["gap_prop"] and small["inv_prop"] == full["inv_prop"]
    assert small["subst_rates"].tobytes() == full["subst_rates"].tobytes()
    with partition(product, res.rows, cmap, S, res.weights) as inst:
        assert product.empirical_subst_rates(inst.p).tobytes() == small["subst_rates"].tobytes()


@pytest.mark.parametrize("states, coded", [(4, True), (20, True), (20, False)])
def test_likelihood_path_untouched(product, states, coded):
    inst = pc.build_instance(product, states=states, rate_cats=4, ntips=9, nsites=300, coded=coded)
    with inst:
        t = inst.tree
        before = pc.full_traversal(inst)
        assert np.isfinite(before)
        assert product.empirical_frequencies(inst.p) is not None
        assert product.empirical_subst_rates(inst.p) is not None
        assert np.isfinite(product.empirical_invariant_sites(inst.p))
        edge = inst.edge_lnl(t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix)
        edge = edge[0] if isinstance(edge, tuple) else edge
        assert np.float64(edge).tobytes() == np.float64(before).tobytes()
        assert np.float64(pc.full_traversal(inst)).tobytes() == np.float64(before).tobytes()
