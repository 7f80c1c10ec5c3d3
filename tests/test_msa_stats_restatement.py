"""Empirical frequencies, exchangeabilities, p-inv and alignment statistics (include/pllhip.h: pllhip_empirical_*,
pllhip_msa_compute_stats), restated in plain Python with exact arithmetic: integers for every count, fractions for the
frequencies, rounded to a double once.  tests/test_msa_stats_gpu.py compares the device against these functions.

The restatement is pinned to pll-modules by tests/golden/msa_stats_fixtures.json (recorded by
tests/golden/record_msa_stats.c against the CPU oracle): frequencies, p-inv and everything of the alignment form
except the exchangeabilities.  The reference resets only half of its per-column counter (its memset counts
sizeof(unsigned) per state, the counters are size_t), so for the exchangeabilities the restatement alone is the
definition -- counts reset for every column -- and one test shows that both agree where the defect cannot act.

The library tests at the end load the product library without a device: symbols, parameter errors, and the
duplicate search, which is host work."""
import ctypes as C
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import pllhip_ctypes as pc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "msa_stats_fixtures.json")
PLL_ERROR_PARAM_INVALID, PLL_ERROR_MSA_MAP_INVALID = 113, 132


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def masks_of(rows, charmap):
    """[T, L] uint64 state masks of rows (bytes per taxon) under a 256-entry character -> state map"""
    cmap = np.asarray([int(x) for x in charmap], dtype=np.uint64)
    return cmap[np.stack([np.frombuffer(bytes(r), dtype=np.uint8) for r in rows])]


def full_mask(S):
    return (1 << S) - 1


def _popcounts(masks):
    return np.asarray([bin(int(m)).count("1") for m in masks.ravel()], dtype=np.int64).reshape(masks.shape)


def _bits(masks, S):
    """[T, L, S] int64: bit k of every mask"""
    return np.stack([((masks >> np.uint64(k)) & np.uint64(1)).astype(np.int64) for k in range(S)], axis=-1)


def frequencies(masks, weights, S, with_gaps):
    """every character adds w / popcount to each state of its mask; with_gaps (the partition form): gaps included,
    over sum(w) * tips; else (the alignment form) gaps ignored, over sum(w) * tips - gap weight"""
    T, L = masks.shape
    w = [int(x) for x in weights]
    full = full_mask(S)
    table = {}                                        # mask -> weight of its characters
    for t in range(T):
        for n in range(L):
            m = int(masks[t, n])
            table[m] = table.get(m, 0) + w[n]
    total = sum(w) * T - (0 if with_gaps else table.get(full, 0))
    out = []
    for k in range(S):
        acc = Fraction(0)
        for m, weight in table.items():
            if (m >> k) & 1 and (with_gaps or m != full):
                acc += Fraction(weight, bin(m).count("1"))
        out.append(float(acc / total) if total else float("nan"))
    return np.asarray(out)


def pair_counts(masks, weights, S, gaps=None):
    """pair[i][j] (Python integers, i < j, row-major): per column cnt[k] = characters that are no gap and contain k,
    pair[i][j] += cnt[i] * cnt[j] * w -- the counts start from zero in every column"""
    T, L = masks.shape
    gaps = (masks == np.uint64(full_mask(S))) if gaps is None else gaps
    cnt = (_bits(masks, S) * (~gaps)[:, :, None]).sum(axis=0)            # [L, S], <= T
    w = np.asarray([int(x) for x in weights], dtype=object)
    assert T * T * int(max(w, default=0)) < 2 ** 62                     # each product is exact in int64 ...
    pairs = []
    for i in range(S):
        for j in range(i + 1, S):
            pairs.append(int(np.sum((cnt[:, i] * cnt[:, j]).astype(object) * w)))   # ... and the sum is Python's
    return pairs


def rates_from_pairs(pairs):
    """pll_msa.c:264-279: the same double operations"""
    last = float(pairs[-1])
    if last < 1e-7:
        last = 1.0
    out = [min(max(float(p) / last, 0.01), 50.0) for p in pairs]
    out[-1] = 1.0
    return np.asarray(out)


def subst_rates(masks, weights, S, gaps=None):
    return rates_from_pairs(pair_counts(masks, weights, S, gaps))


def invariant_partition(masks, weights):
    """pll_update_invariant_sites' rule: the characters of the column share any state (an all-gap column counts)"""
    common = np.bitwise_and.reduce(masks, axis=0)
    w = [int(x) for x in weights]
    inv = sum(w[n] for n in range(len(w)) if int(common[n]) != 0)
    return float(inv) / float(sum(w))


def vector_masks(vectors):
    """tips as vectors [T, L, S]: (masks {k: v[k] > 0}, gap = every entry >= 1e-7 -- what the rates skip)"""
    T, L, S = vectors.shape
    masks = np.zeros((T, L), dtype=np.uint64)
    for k in range(S):
        masks |= (vectors[:, :, k] > 0).astype(np.uint64) << np.uint64(k)
    return masks, np.all(vectors >= 1e-7, axis=2)


def vector_frequencies(vectors, weights):
    """true probability vectors: every character adds w * v[k] / sum(v); over sum(w) * tips"""
    T, L, S = vectors.shape
    w = [int(x) for x in weights]
    acc = [Fraction(0)] * S
    for t in range(T):
        for n in range(L):
            v = [Fraction(float(x)) for x in vectors[t, n]]
            tot = sum(v)
            for k in range(S):
                acc[k] += w[n] * v[k] / tot
    return np.asarray([float(a / (sum(w) * T)) for a in acc])


def duplicate_pairs(strings):
    """(first occurrence, later copy), ordered by first occurrence, then by copy"""
    first, pairs = {}, []
    for j, s in enumerate(strings):
        if s in first:
            pairs.append((first[s], j))
        else:
            first[s] = j
    return sorted(pairs)


class UnknownState(Exception):
    """a character that maps to 0: (sequence, position), 1-based, the first in sequence-major order"""


def msa_stats(rows, S, charmap, weights=None, mask=pc.MSA_STATS_ALL, labels=None):
    """pllhip_msa_compute_stats: the dict PllLib.msa_compute_stats returns"""
    rows = [bytes(r) for r in rows]
    T, L = len(rows), len(rows[0])
    out = {"states": S, "dup_taxa_pairs": [], "dup_seqs_pairs": [], "gap_prop": 0.0, "gap_seqs": [], "gap_cols": [],
           "inv_prop": 0.0, "inv_cols": [], "freqs": None, "subst_rates": None}
    if mask & pc.MSA_STATS_DUP_TAXA:
        out["dup_taxa_pairs"] = duplicate_pairs([b"t%d" % t for t in range(T)] if labels is None else list(labels))
    if mask & pc.MSA_STATS_DUP_SEQS:
        out["dup_seqs_pairs"] = duplicate_pairs(rows)
    if not mask & ~(pc.MSA_STATS_DUP_TAXA | pc.MSA_STATS_DUP_SEQS):
        return out
    masks = masks_of(rows, charmap)
    bad = np.argwhere(masks == 0)
    if len(bad):
        raise UnknownState((int(bad[0][0]) + 1, int(bad[0][1]) + 1))
    w = [1] * L if weights is None else [int(x) for x in weights]
    gaps = masks == np.uint64(full_mask(S))
    sum_w = sum(w)
    gap_weight = sum(w[n] * int(gaps[:, n].sum()) for n in range(L))
    if mask & pc.MSA_STATS_SUBST_RATES:
        out["subst_rates"] = subst_rates(masks, w, S)
    if mask & pc.MSA_STATS_FREQS:
        out["freqs"] = frequencies(masks, w, S, with_gaps=False)
    if mask & pc.MSA_STATS_GAP_PROP:
        out["gap_prop"] = float(gap_weight) / float(sum_w * T)
    if mask & pc.MSA_STATS_GAP_COLS:
        out["gap_cols"] = [n for n in range(L) if gaps[:, n].all()]
    if mask & pc.MSA_STATS_GAP_SEQS:
        out["gap_seqs"] = [t for t in range(T) if sum(w[n] for n in range(L) if gaps[t, n]) == sum_w]
    if mask & (pc.MSA_STATS_INV_COLS | pc.MSA_STATS_INV_PROP):
        common = np.bitwise_and.reduce(masks, axis=0)
        out["inv_cols"] = [n for n in range(L) if bin(int(common[n])).count("1") == 1]
        out["inv_prop"] = float(sum(w[n] for n in out["inv_cols"])) / float(sum_w)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against the reference's recorded results
# ---------------------------------------------------------------------------------------------------------------------
def load_cases():
    if not os.path.exists(FIXTURE):
        return []
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


CASES = load_cases()


def close_sum(got, want, terms):
    """a sum of `terms` non-negative terms in any order: (terms + 2) * 2^-52 relative"""
    return abs(got - want) <= (terms + 2) * 2.0 ** -52 * abs(want)


def test_fixture_is_there_and_covers_the_cases():
    names = [c["name"] for c in CASES]
    assert len(names) >= 5, "tests/golden/msa_stats_fixtures.json is missing or short"
    assert os.path.getsize(FIXTURE) < 100_000
    assert any(c["stats"]["gap_cols"] for c in CASES) and any(c["stats"]["gap_seqs"] for c in CASES)
    assert any(c["stats"]["dup_seqs_pairs"] for c in CASES) and any(c["stats"]["dup_taxa_pairs"] for c in CASES)
    assert any(p["attributes"] & pc.PLL_ATTRIB_PATTERN_TIP == 0 for c in CASES for p in c["partitions"])
    assert {c["states"] for c in CASES} >= {2, 4, 20}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_alignment_form_against_the_reference(product_nogpu, case):
    rows = [r.encode() for r in case["rows"]]
    labels = [s.encode() for s in case["labels"]]
    S, want = case["states"], case["stats"]
    got = msa_stats(rows, S, product_nogpu.char_map(case["map"]), case["weights"], pc.MSA_STATS_ALL, labels)
    pairs = lambda flat: [(flat[2 * i], flat[2 * i + 1]) for i in range(len(flat) // 2)]
    assert got["dup_taxa_pairs"] == pairs(want["dup_taxa_pairs"])
    assert got["dup_seqs_pairs"] == pairs(want["dup_seqs_pairs"])
    assert got["gap_seqs"] == want["gap_seqs"] and got["gap_cols"] == want["gap_cols"]
    assert got["inv_cols"] == want["inv_cols"]
    terms = len(rows) * len(rows[0])
    assert close_sum(got["gap_prop"], want["gap_prop"], terms)
    assert close_sum(got["inv_prop"], want["inv_prop"], terms)
    for k in range(S):
        assert close_sum(got["freqs"][k], want["freqs"][k], terms), (k, got["freqs"][k], want["freqs"][k])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_partition_form_against_the_reference(product_nogpu, case):
    rows = [r.encode() for r in case["rows"]]
    S = case["states"]
    masks = masks_of(rows, product_nogpu.char_map(case["map"]))
    terms = masks.size
    assert case["partitions"]
    for part in case["partitions"]:                     # (coded tips and 0/1 vectors: the same numbers)
        got = frequencies(masks, case["weights"], S, with_gaps=True)
        for k in range(S):
            assert close_sum(got[k], part["freqs"][k], terms), (part["attributes"], k, got[k], part["freqs"][k])
        assert close_sum(invariant_partition(masks, case["weights"]), part["pinv"], terms)
        if not part["attributes"] & pc.PLL_ATTRIB_PATTERN_TIP:
            vectors = _bits(masks, S).astype(np.float64)
            vm, vgaps = vector_masks(vectors)
            assert np.array_equal(vm, masks) and np.array_equal(vgaps, masks == np.uint64(full_mask(S)))
            vf = vector_frequencies(vectors, case["weights"])
            for k in range(S):
                assert close_sum(vf[k], part["freqs"][k], terms)


def reference_pair_counts(masks, weights, S):
    """the reference's loop as it runs: its per-column reset clears 4 * S bytes of S 8-byte counters, so only the
    lower half of the states starts a column from zero (little-endian: of an odd S, the low word of the middle one)"""
    T, L = masks.shape
    full = full_mask(S)
    counter = [0] * S
    pair = [[0] * S for _ in range(S)]
    for n in range(L):
        for k in range(S // 2):
            counter[k] = 0
        if S % 2:
            counter[S // 2] &= ~0xffffffff
        for t in range(T):
            m = int(masks[t, n])
            if m == full:
                continue
            for k in range(S):
                counter[k] += (m >> k) & 1
        for i in range(S):
            for j in range(i + 1, S):
                pair[i][j] += counter[i] * counter[j] * int(weights[n])
    return [pair[i][j] for i in range(S) for j in range(i + 1, S)]


@pytest.mark.parametrize("map_name, S, column", [("pll_map_nt", 4, b"ACGTRYN-acKT"), ("pll_map_aa", 20, b"ARNDBZX-VVWY"),
                                                 ("pll_map_bin", 2, b"0101-1")])
def test_rates_equal_the_reference_formula_on_a_single_column(product_nogpu, map_name, S, column):
    cmap = product_nogpu.char_map(map_name)
    one = masks_of([bytes([c]) for c in column], cmap)                   # every character a sequence: one column
    assert pair_counts(one, [7], S) == reference_pair_counts(one, [7], S)
    assert np.array_equal(subst_rates(one, [7], S), rates_from_pairs(reference_pair_counts(one, [7], S)))
    # ... and with a second column the upper half of the reference's counter carries the first one over
    two = np.concatenate([one, one], axis=1)
    assert pair_counts(two, [7, 7], S) == [2 * p for p in pair_counts(one, [7], S)]
    assert pair_counts(two, [7, 7], S) != reference_pair_counts(two, [7, 7], S)


def test_rate_rules():
    # pair[S-2][S-1] == 0: the divisor falls back to 1; both clamps; the last entry is 1
    assert list(rates_from_pairs([3, 0, 200, 0, 7, 0])) == [3.0, 0.01, 50.0, 0.01, 7.0, 1.0]
    assert list(rates_from_pairs([1, 1000, 5, 5, 5, 10])) == [0.1, 50.0, 0.5, 0.5, 0.5, 1.0]


# ---------------------------------------------------------------------------------------------------------------------
# the library, without a device
# ---------------------------------------------------------------------------------------------------------------------
NAMES = ["pllhip_empirical_frequencies", "pllhip_empirical_subst_rates", "pllhip_empirical_invariant_sites",
         "pllhip_msa_compute_stats", "pllhip_msa_destroy_stats"]


def test_symbols_are_exported(product_nogpu):
    missing = [n for n in NAMES if not hasattr(product_nogpu.lib, n)]
    assert not missing, missing
    assert all(n in pc.PLLHIP_H_FUNCTIONS for n in NAMES)
    # a client that also links pll-modules' pll_msa.c must not get duplicate symbols
    assert not [n for n in ("pllmod_msa_compute_stats", "pllmod_msa_empirical_frequencies") if hasattr(product_nogpu.lib, n)]


def test_parameter_errors_come_before_any_device_call(product_nogpu):
    lib, L = product_nogpu, product_nogpu.lib
    cmap = (C.c_ulonglong * 256)(*[int(x) for x in lib.char_map("pll_map_nt")])
    lib.errno = 0
    assert not L.pllhip_empirical_frequencies(None) and lib.errno == PLL_ERROR_PARAM_INVALID
    lib.errno = 0
    assert not L.pllhip_empirical_subst_rates(None) and lib.errno == PLL_ERROR_PARAM_INVALID
    lib.errno = 0
    assert L.pllhip_empirical_invariant_sites(None) == -np.inf and lib.errno == PLL_ERROR_PARAM_INVALID
    buf = C.create_string_buffer(b"ACGT", 5)
    seqs = (C.c_void_p * 1)(C.addressof(buf))
    msa = pc.Msa(1, 4, seqs, None)
    for args in ((None, 4, cmap), (C.byref(msa), 4, None), (C.byref(msa), 1, cmap), (C.byref(msa), 65, cmap)):
        lib.errno = 0
        assert not L.pllhip_msa_compute_stats(args[0], args[1], args[2], None, pc.MSA_STATS_FREQS)
        assert lib.errno == PLL_ERROR_PARAM_INVALID, (args[1], lib.errno, lib.errmsg)
    L.pllhip_msa_destroy_stats(None)


def test_duplicates_need_no_device(product_nogpu):
    rows = [b"ACGTAC", b"AC-TAC", b"ACGTAC", b"TTTTTT", b"ACGTAC", b"AC-TAA", b"GGGGGG"]     # 0 = 2 = 4
    labels = [b"a", b"b", b"c", b"d", b"e", b"b", b"f"]                                       # 1 = 5
    cmap = product_nogpu.char_map("pll_map_nt")
    mask = pc.MSA_STATS_DUP_TAXA | pc.MSA_STATS_DUP_SEQS
    want = msa_stats(rows, 4, cmap, None, mask, labels)
    assert want["dup_seqs_pairs"] == [(0, 2), (0, 4)] and want["dup_taxa_pairs"] == [(1, 5)]
    got = product_nogpu.msa_compute_stats(rows, 4, cmap, None, mask, labels)
    assert got is not None, (product_nogpu.errno, product_nogpu.errmsg)
    assert got["dup_seqs_pairs"] == want["dup_seqs_pairs"] and got["dup_taxa_pairs"] == want["dup_taxa_pairs"]
    assert got["states"] == 4 and got["freqs"] is None and got["subst_rates"] is None
    assert got["gap_cols"] == [] and got["gap_seqs"] == [] and got["inv_cols"] == []
    for single in (pc.MSA_STATS_DUP_TAXA, pc.MSA_STATS_DUP_SEQS):
        one = product_nogpu.msa_compute_stats(rows, 4, cmap, None, single, labels)
        assert one["dup_seqs_pairs"] == (want["dup_seqs_pairs"] if single == pc.MSA_STATS_DUP_SEQS else [])
        assert one["dup_taxa_pairs"] == (want["dup_taxa_pairs"] if single == pc.MSA_STATS_DUP_TAXA else [])
