"""pll_compress_site_patterns / pll_compress_site_patterns_msa on the device (csrc/pll_compress_dev.hip) against
numpy: two sites are one pattern iff their characters map to equal states in every sequence; patterns come in the
order of their first occurrence and keep its characters.  Everything is compared for equality."""
import os

import numpy as np
import pytest

import pllhip_ctypes as pc

pytestmark = pytest.mark.gpu

PLL_ERROR_PARAM_INVALID, PLL_ERROR_TIPDATA_ILLEGALSTATE = 113, 114


def reference(rows, charmap):
    """(compressed rows [T, P] uint8, weights [P], site -> pattern [L]) of rows [T, L] uint8"""
    cmap = np.asarray(list(charmap), dtype=np.uint64)
    _, dense = np.unique(cmap, return_inverse=True)              # equal map value <=> equal small code
    states = dense.astype(np.uint8)[rows]
    T, L = rows.shape
    if T == 2:
        keys = np.ascontiguousarray(states.T).view(np.uint16).ravel()
    else:
        keys = np.ascontiguousarray(states.T).view(np.dtype((np.void, T))).ravel()
    _, first, inverse, counts = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")                     # patterns by first occurrence
    number = np.empty(len(order), dtype=np.int64)
    number[order] = np.arange(len(order))
    return rows[:, first[order]], counts[order].astype(np.uint32), number[inverse.ravel()].astype(np.uint32)


def check(lib, rows, charmap, msa_form=True):
    res = lib.compress_site_patterns([r.tobytes() for r in rows], charmap, msa_form=msa_form)
    assert res.ok, (res.errno, res.errmsg)
    want_rows, want_w, want_map = reference(rows, charmap)
    P = want_rows.shape[1]
    assert res.length == P
    assert int(res.weights.sum(dtype=np.uint64)) == rows.shape[1]
    assert np.array_equal(res.weights, want_w)
    for t in range(rows.shape[0]):
        assert res.rows[t] == want_rows[t].tobytes(), t          # P characters, then the NUL
    if msa_form:
        assert np.array_equal(res.site_pattern_map, want_map)
    return res


def draw(rng, alphabet, T, L, npatterns):
    """[T, L] uint8: every column is one of `npatterns` random columns over `alphabet`"""
    base = rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=(T, npatterns))
    return np.ascontiguousarray(base[:, rng.integers(0, npatterns, size=L)])


DNA = b"ACGTacgtACGTacgt-N?nRYrykM"
AA = b"ARNDCQEGHILKMFPSTWYVarndcqeghilkmfpstwyvBZX*-?bzx"


@pytest.mark.parametrize("L", [1, 63, 64, 65, 257, 1000])
def test_dna_small(product, L):
    rng = np.random.default_rng(100 + L)
    rows = draw(rng, DNA, 7, L, 40)
    res = check(product, rows, product.char_map("pll_map_nt"), msa_form=True)
    plain = check(product, rows, product.char_map("pll_map_nt"), msa_form=False)
    assert plain.rows == res.rows and np.array_equal(plain.weights, res.weights)


def test_case_and_gap_characters_merge(product):
    rows = np.frombuffer(b"AaCN-?G" b"TtGn?-G", dtype=np.uint8).reshape(2, 7)
    res = check(product, rows, product.char_map("pll_map_nt"))
    assert res.rows == [b"ACNG", b"TGnG"] and list(res.weights) == [2, 1, 3, 1]
    assert list(res.site_pattern_map) == [0, 0, 1, 2, 2, 2, 3]


def test_one_taxon(product):
    rng = np.random.default_rng(3)
    check(product, draw(rng, DNA, 1, 777, 30), product.char_map("pll_map_nt"))


def test_all_columns_identical(product):
    rows = np.repeat(np.frombuffer(b"ACgT-", dtype=np.uint8).reshape(5, 1), 100_000, axis=1)
    res = check(product, rows, product.char_map("pll_map_nt"))
    assert res.length == 1 and list(res.weights) == [100_000]


def test_all_columns_distinct(product):
    # 4096 distinct columns of 6 taxa over A C G T: column s spells s in base 4
    s = np.arange(4096)
    rows = np.frombuffer(b"ACGT", dtype=np.uint8)[np.stack([(s >> (2 * t)) & 3 for t in range(6)])]
    rows = np.ascontiguousarray(rows[:, np.random.default_rng(4).permutation(4096)])
    res = check(product, rows, product.char_map("pll_map_nt"))
    assert res.length == 4096 and np.all(res.weights == 1)
    assert [r for r in res.rows] == [r.tobytes() for r in rows]


def test_protein_map(product):
    rng = np.random.default_rng(5)
    rows = draw(rng, AA, 6, 500, 60)
    check(product, rows, product.char_map("pll_map_aa"))
    merge = np.frombuffer(b"X*-?x" b"AAAAA", dtype=np.uint8).reshape(2, 5)
    res = check(product, merge, product.char_map("pll_map_aa"))
    assert res.length == 1 and res.rows == [b"X", b"A"]


def test_beyond_one_scan_level_with_heavy_contention(product):
    """5 M sites: more than 1024 scan tiles; at most 256 patterns: every table slot is shared by ~20 k sites"""
    rng = np.random.default_rng(6)
    rows = draw(rng, b"ACGTacgtN-", 2, 5_000_000, 256)
    res = check(product, rows, product.char_map("pll_map_nt"))
    assert res.length <= 256


@pytest.fixture(scope="module")
def many_groups(product):
    """50 x 200 000 from 20 000 distinct columns: a multi-block grid, several scan tiles, a well-filled table"""
    rng = np.random.default_rng(7)
    rows = draw(rng, DNA, 50, 200_000, 20_000)
    cmap = product.char_map("pll_map_nt")
    first = product.compress_site_patterns([r.tobytes() for r in rows], cmap, msa_form=True)
    return rows, reference(rows, cmap), first


def test_many_groups(many_groups):
    rows, (want_rows, want_w, want_map), res = many_groups
    assert res.ok, (res.errno, res.errmsg)
    assert res.length == want_rows.shape[1] > 15_000
    assert np.array_equal(res.weights, want_w) and np.array_equal(res.site_pattern_map, want_map)
    assert res.rows == [r.tobytes() for r in want_rows]


def test_reproducible_from_run_to_run(product, many_groups):
    rows, _, first = many_groups
    again = product.compress_site_patterns([r.tobytes() for r in rows], product.char_map("pll_map_nt"), msa_form=True)
    assert first.ok and again.ok
    assert again.length == first.length and again.rows == first.rows
    assert again.weights.tobytes() == first.weights.tobytes()
    assert again.site_pattern_map.tobytes() == first.site_pattern_map.tobytes()


def test_result_does_not_depend_on_the_hash(product):
    """PLLHIP_COMPRESS_HASH_BITS=0: every site probes from slot 0 and every tag matches, so the full compare and the
    probing alone produce the result"""
    rng = np.random.default_rng(8)
    rows = draw(rng, DNA, 5, 300, 100)
    saved = os.environ.get("PLLHIP_COMPRESS_HASH_BITS")
    results = []
    try:
        for bits in ("0", "3", None):
            if bits is None:
                os.environ.pop("PLLHIP_COMPRESS_HASH_BITS", None)
            else:
                os.environ["PLLHIP_COMPRESS_HASH_BITS"] = bits
            results.append(check(product, rows, product.char_map("pll_map_nt")))
    finally:
        if saved is None:
            os.environ.pop("PLLHIP_COMPRESS_HASH_BITS", None)
        else:
            os.environ["PLLHIP_COMPRESS_HASH_BITS"] = saved
    for r in results[1:]:
        assert r.rows == results[0].rows and r.weights.tobytes() == results[0].weights.tobytes()
        assert r.site_pattern_map.tobytes() == results[0].site_pattern_map.tobytes()
    # the knob was read, and the paths it is there for ran (pllhip_compress_last_counts)
    zero, three, full = results
    L, P = rows.shape[1], full.length
    print("probe steps / compares: 0 bits", (zero.probe_steps, zero.compares), "3 bits", (three.probe_steps, three.compares),
          "all bits", (full.probe_steps, full.compares))
    # all bits (seeded data: no two distinct columns share a tag): one compare per site that joined a group
    assert full.compares == L - P
    # 0 bits: one chain of P slots from slot 0 and every tag matches.  The k-th pattern of the chain is reached over
    # k slots by each of its sites (>= 1), and every slot passed over is one compare that said "unequal"
    assert zero.probe_steps >= P * (P - 1) // 2
    assert zero.compares == zero.probe_steps + (L - P)
    # 3 bits: 8 first slots for P patterns, so they fill P consecutive slots that begin at slot 7 at the latest: the
    # k-th of them (k >= 8) is reached over at least k - 7 slots by each of its sites.  With all bits the table of
    # 1024 slots holds P < 100 entries at hashed places: linear probing at a load below 0.1 passes over about
    # load / 2 slots per lookup, a few dozen over the 300 sites
    assert three.probe_steps >= (P - 8) * (P - 7) // 2 > full.probe_steps
    assert three.compares >= L - P


def test_illegal_character(product):
    rng = np.random.default_rng(9)
    rows = draw(rng, DNA, 6, 3000, 50).copy()
    rows[4, 2900] = ord("#")
    rows[2, 17] = ord("!")                       # the first in sequence-major order
    rows[2, 2000] = ord("#")
    rows[5, 3] = ord("#")
    for msa_form in (False, True):
        res = product.compress_site_patterns([r.tobytes() for r in rows], product.char_map("pll_map_nt"),
                                             msa_form=msa_form)
        assert not res.ok
        assert res.errno == PLL_ERROR_TIPDATA_ILLEGALSTATE
        assert "'!'" in res.errmsg and "sequence 2, site 17" in res.errmsg, res.errmsg
        assert res.length == 3000
        assert res.rows == [r.tobytes() for r in rows]


def test_bad_parameters(product):
    cmap = product.char_map("pll_map_nt")
    for kw in ({"count": 0}, {"length": 0}, {"count": -1}, {"length": -5}):
        for msa_form in (False, True):
            res = product.compress_site_patterns([b"ACGT", b"AACC"], cmap, msa_form=msa_form, **kw)
            assert not res.ok and res.errno == PLL_ERROR_PARAM_INVALID, (kw, res.errno, res.errmsg)
            assert res.rows == [b"ACGT", b"AACC"] and res.length == kw.get("length", 4)
    product.errno = 0
    assert not product.lib.pll_compress_site_patterns(None, cmap, 2, None)
    assert product.errno == PLL_ERROR_PARAM_INVALID
    assert not product.lib.pll_compress_site_patterns_msa(None, cmap, None)
    assert product.errno == PLL_ERROR_PARAM_INVALID


def _partition(lib, tree, rows, weights):
    inst = pc.Instance(lib, len(rows), 4, len(rows[0]), 4, attributes=pc.PLL_ATTRIB_PATTERN_TIP)
    inst.set_model(pc.DNA_GTR_RATES, pc.DNA_FREQS, lib.gamma_cats(0.841, 4))
    for t, r in enumerate(rows):
        inst.set_tip_states(t, lib.char_map("pll_map_nt"), r)
    inst.set_pattern_weights(weights)
    inst.tree = tree
    return inst


def _lnl(inst):
    total = pc.full_traversal(inst)
    t = inst.tree
    _, persite = inst.edge_lnl(t.root_a, t.scaler_of(t.root_a), t.root_b, t.scaler_of(t.root_b), t.root_matrix,
                               persite=True)
    return total, persite


def test_end_to_end_phylip_compress_likelihood(product, tmp_path):
    lib = product
    T, N = 12, 2048
    rng = np.random.default_rng(10)
    rows = draw(rng, b"ACGTacgtN-RY", T, N, 300)
    path = tmp_path / "aln.phy"
    path.write_text("%d %d\n" % (T, N) + "".join("t%d %s\n" % (t, rows[t].tobytes().decode()) for t in range(T)))
    msa = lib.phylip_load(path)
    assert msa, (lib.errno, lib.errmsg)
    try:
        count, length, labels, original = lib.msa_contents(msa)
        assert (count, length) == (T, N) and original == [r.tobytes() for r in rows]
        spm = np.zeros(N, dtype=np.uint32)
        w = lib.lib.pll_compress_site_patterns_msa(msa, lib.char_map("pll_map_nt"), spm.ctypes.data_as(pc.c_uint_p))
        assert w, (lib.errno, lib.errmsg)
        _, P, _, compressed = lib.msa_contents(msa)
        weights = np.ctypeslib.as_array(w, shape=(P,)).copy()
        pc._libc_free(w)
    finally:
        lib.lib.pll_msa_destroy(msa)
    assert P < N and int(weights.sum()) == N and all(len(r) == P for r in compressed)
    tree = pc.Tree(T)
    with _partition(lib, tree, original, np.ones(N, dtype=np.uint32)) as full, \
            _partition(lib, tree, compressed, weights) as small:
        lnl_full, site_full = _lnl(full)
        lnl_small, site_small = _lnl(small)
    bound = 1e-6 * N                              # the bar of smoke(): the sums run in another order
    print(f"lnL original {lnl_full:.10f} compressed {lnl_small:.10f} diff {abs(lnl_full - lnl_small):.3e}")
    print(f"max per-site diff {np.max(np.abs(site_full - site_small[spm])):.3e}")
    assert np.isfinite(lnl_full) and abs(lnl_full - lnl_small) < bound
    assert np.max(np.abs(site_full - site_small[spm])) < bound
