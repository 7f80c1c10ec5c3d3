"""The alignment readers of the product library (csrc/host/pll_msa_io.c): pll_fasta_*, pll_phylip_load,
pll_msa_destroy.  Host code only: no GPU."""
import numpy as np
import pytest

import pllhip_ctypes as pc

PLL_ERROR_FILE_OPEN, PLL_ERROR_FILE_EOF = 100, 102
PLL_ERROR_FASTA_ILLEGALCHAR, PLL_ERROR_FASTA_UNPRINTABLECHAR, PLL_ERROR_FASTA_INVALIDHEADER = 201, 202, 203
PLL_ERROR_PHYLIP_SYNTAX, PLL_ERROR_PHYLIP_LONGSEQ, PLL_ERROR_PHYLIP_NONALIGNED, PLL_ERROR_PHYLIP_ILLEGALCHAR = \
    231, 232, 233, 234

LONG_SEQ = ("ACGTTGCAAC" * 500)[:4999]           # one line, longer than the 2048-byte buffer of pll_fasta_t
FASTA = (b">first record  with blanks\r\n"
         b"ACGTacgt\r\n"
         b"nn--??\r\n"
         b"\r\n"
         b"TTGA\r\n"
         b">second\r\n" + LONG_SEQ.encode() + b"\r\n"
         b">third|x\r\n"
         b"ac gt\r\n"
         b"\tRYKM\r\n")
FASTA_RECORDS = [(b"first record  with blanks", b"ACGTacgtnn--??TTGA"), (b"second", LONG_SEQ.encode()),
                 (b"third|x", b"acgtRYKM")]


def _read_all(lib, fd):
    out = []
    while True:
        lib.errno = 0
        rec = lib.fasta_getnext(fd)
        if rec is None:
            return out
        out.append(rec)


def test_fasta_records_rewind_and_eof(product_nogpu, tmp_path):
    lib = product_nogpu
    path = tmp_path / "a.fasta"
    path.write_bytes(FASTA)
    fd = lib.fasta_open(path)
    assert fd, (lib.errno, lib.errmsg)
    try:
        for attempt in range(2):
            recs = _read_all(lib, fd)
            # the end of the file is exactly PLL_ERROR_FILE_EOF (what test/src/tree/treemove-spr.c:204 tests for)
            assert lib.errno == PLL_ERROR_FILE_EOF, (attempt, lib.errno, lib.errmsg)
            assert len(recs) == 3
            for k, ((head, head_len, seq, seq_len, seqno), (want_head, want_seq)) in enumerate(zip(recs, FASTA_RECORDS)):
                assert head == want_head and head_len == len(want_head)
                assert seq == want_seq and seq_len == len(want_seq)
                assert seqno == k
            # a second call at the end of the file says the same again
            assert lib.fasta_getnext(fd) is None and lib.errno == PLL_ERROR_FILE_EOF
            assert lib.lib.pll_fasta_rewind(fd)
    finally:
        lib.lib.pll_fasta_close(fd)


def test_fasta_without_final_newline_and_empty_sequence(product_nogpu, tmp_path):
    lib = product_nogpu
    path = tmp_path / "b.fasta"
    path.write_bytes(b"\n>empty\n>last\nAC\nGT")
    fd = lib.fasta_open(path)
    assert fd
    try:
        recs = _read_all(lib, fd)
        assert lib.errno == PLL_ERROR_FILE_EOF
        assert [(r[0], r[2], r[3], r[4]) for r in recs] == [(b"empty", b"", 0, 0), (b"last", b"ACGT", 4, 1)]
    finally:
        lib.lib.pll_fasta_close(fd)


def test_fasta_illegal_character_names_the_line(product_nogpu, tmp_path):
    lib = product_nogpu
    path = tmp_path / "c.fasta"
    path.write_bytes(b">a\nACGT\nAC\n>b\nAC\nGG#T\nAA\n")
    fd = lib.fasta_open(path)
    assert fd
    try:
        assert lib.fasta_getnext(fd)[2] == b"ACGTAC"
        lib.errno = 0
        assert lib.fasta_getnext(fd) is None
        assert lib.errno == PLL_ERROR_FASTA_ILLEGALCHAR
        assert "'#'" in lib.errmsg and "line 6" in lib.errmsg, lib.errmsg
    finally:
        lib.lib.pll_fasta_close(fd)


def test_fasta_nul_byte_is_fatal(product_nogpu, tmp_path):
    lib = product_nogpu
    path = tmp_path / "d.fasta"
    path.write_bytes(b">a\nAC\x00GT\n")
    fd = lib.fasta_open(path)
    assert fd
    try:
        lib.errno = 0
        assert lib.fasta_getnext(fd) is None
        assert lib.errno == PLL_ERROR_FASTA_UNPRINTABLECHAR
    finally:
        lib.lib.pll_fasta_close(fd)


def test_fasta_missing_file_and_bad_header(product_nogpu, tmp_path):
    lib = product_nogpu
    lib.errno = 0
    assert not lib.fasta_open(tmp_path / "does_not_exist.fasta")
    assert lib.errno == PLL_ERROR_FILE_OPEN
    path = tmp_path / "e.fasta"
    path.write_bytes(b"ACGT\n>a\nAC\n")
    fd = lib.fasta_open(path)
    assert fd
    try:
        lib.errno = 0
        assert lib.fasta_getnext(fd) is None
        assert lib.errno == PLL_ERROR_FASTA_INVALIDHEADER
    finally:
        lib.lib.pll_fasta_close(fd)


def test_fasta_custom_status_table(product_nogpu, tmp_path):
    """status 3 strips silently, whatever the character"""
    lib = product_nogpu
    status = list(lib.char_map("pll_map_fasta"))
    status[ord("#")] = 3
    path = tmp_path / "f.fasta"
    path.write_bytes(b">a\nAC#G#T\n")
    fd = lib.fasta_open(path, status)
    assert fd
    try:
        assert lib.fasta_getnext(fd)[2] == b"ACGT"
    finally:
        lib.lib.pll_fasta_close(fd)


# --- PHYLIP -------------------------------------------------------------------------------------------------------

def _alignment():
    rng = np.random.default_rng(5)
    seqs = ["".join(rng.choice(list("ACGTacgtNRY-?"), size=37)) for _ in range(5)]
    labels = ["taxon_%d|x" % i for i in range(5)]
    return labels, seqs


def _sequential(labels, seqs):
    """sequences wrapped over lines of 11, with blanks inside, the first chunk on the label's line or the next"""
    out = [" 5   37 "]
    for k, (lab, s) in enumerate(zip(labels, seqs)):
        chunks = [s[i:i + 11] for i in range(0, len(s), 11)]
        chunks = [c[:4] + " " + c[4:] for c in chunks]
        if k % 2:
            out.append(lab)
            out.extend("  " + c for c in chunks)
        else:
            out.append(lab + "  " + chunks[0])
            out.extend(chunks[1:])
    return "\n".join(out) + "\n"


def _interleaved(labels, seqs, crlf=False):
    out = ["5 37"]
    for start in range(0, 37, 10):
        for lab, s in zip(labels, seqs):
            out.append((lab + "   " if start == 0 else "") + s[start:start + 10])
        out.append("")
    return ("\r\n" if crlf else "\n").join(out) + "\n"


def _load(lib, tmp_path, text, interleaved, name="x.phy"):
    path = tmp_path / name
    path.write_bytes(text.encode() if isinstance(text, str) else text)
    lib.errno = 0
    msa = lib.phylip_load(path, interleaved)
    if not msa:
        return None
    try:
        return lib.msa_contents(msa)
    finally:
        lib.lib.pll_msa_destroy(msa)


def test_phylip_sequential_and_interleaved_agree(product_nogpu, tmp_path):
    lib = product_nogpu
    labels, seqs = _alignment()
    want = (5, 37, [l.encode() for l in labels], [s.encode() for s in seqs])
    assert _load(lib, tmp_path, _sequential(labels, seqs), False) == want, lib.errmsg
    assert _load(lib, tmp_path, _interleaved(labels, seqs), True) == want, lib.errmsg
    assert _load(lib, tmp_path, _interleaved(labels, seqs, crlf=True), True) == want, lib.errmsg


def test_phylip_one_taxon_per_line_reads_in_both_forms(product_nogpu, tmp_path):
    lib = product_nogpu
    text = "3 6\na ACGTAC\nb AC-TAC\nc NNGTAC\n"
    want = (3, 6, [b"a", b"b", b"c"], [b"ACGTAC", b"AC-TAC", b"NNGTAC"])
    assert _load(lib, tmp_path, text, False) == want
    assert _load(lib, tmp_path, text, True) == want


def test_phylip_short_taxon(product_nogpu, tmp_path):
    lib = product_nogpu
    labels, seqs = _alignment()
    # sequential: the file ends before the last taxon has its sites
    assert _load(lib, tmp_path, _sequential(labels, seqs[:4] + [seqs[4][:30]]), False) is None
    assert lib.errno == PLL_ERROR_PHYLIP_NONALIGNED, lib.errmsg
    # interleaved: any taxon
    assert _load(lib, tmp_path, _interleaved(labels, seqs[:2] + [seqs[2][:35]] + seqs[3:]), True) is None
    assert lib.errno == PLL_ERROR_PHYLIP_NONALIGNED, lib.errmsg
    assert "taxon_2|x" in lib.errmsg, lib.errmsg


def test_phylip_long_taxon(product_nogpu, tmp_path):
    lib = product_nogpu
    labels, seqs = _alignment()
    text = "5 37\n" + "".join("%s %s\n" % (l, s + ("AC" if k == 3 else "")) for k, (l, s) in enumerate(zip(labels, seqs)))
    assert _load(lib, tmp_path, text, False) is None
    assert lib.errno == PLL_ERROR_PHYLIP_LONGSEQ, lib.errmsg
    assert _load(lib, tmp_path, text, True) is None
    assert lib.errno == PLL_ERROR_PHYLIP_LONGSEQ, lib.errmsg
    assert _load(lib, tmp_path, _interleaved(labels, seqs[:1] + [seqs[1] + "A"] + seqs[2:]), True) is None
    assert lib.errno == PLL_ERROR_PHYLIP_LONGSEQ, lib.errmsg


@pytest.mark.parametrize("header", ["5\n", "five 37\n", "5 37 x\n", "0 37\n", "5 -3\n", ""])
def test_phylip_bad_header(product_nogpu, tmp_path, header):
    lib = product_nogpu
    labels, seqs = _alignment()
    body = "".join("%s %s\n" % (l, s) for l, s in zip(labels, seqs))
    for interleaved in (False, True):
        assert _load(lib, tmp_path, header + body, interleaved) is None
        assert lib.errno == PLL_ERROR_PHYLIP_SYNTAX, lib.errmsg


def test_phylip_header_with_many_trailing_blanks(product_nogpu, tmp_path):
    lib = product_nogpu
    text = "3 6" + " " * 400 + "\r\na ACGTAC\nb AC-TAC\nc NNGTAC\n"
    assert _load(lib, tmp_path, text, False) == (3, 6, [b"a", b"b", b"c"], [b"ACGTAC", b"AC-TAC", b"NNGTAC"])
    assert _load(lib, tmp_path, "3 6" + " " * 400 + "x\na ACGTAC\nb AC-TAC\nc NNGTAC\n", False) is None
    assert lib.errno == PLL_ERROR_PHYLIP_SYNTAX


def test_phylip_too_few_records(product_nogpu, tmp_path):
    lib = product_nogpu
    labels, seqs = _alignment()
    body = "".join("%s %s\n" % (l, s) for l, s in zip(labels[:4], seqs[:4]))
    for interleaved in (False, True):
        assert _load(lib, tmp_path, "5 37\n" + body, interleaved) is None
        assert lib.errno == PLL_ERROR_PHYLIP_SYNTAX, lib.errmsg


def test_phylip_illegal_character(product_nogpu, tmp_path):
    lib = product_nogpu
    labels, seqs = _alignment()
    bad = seqs[:2] + [seqs[2][:9] + "#" + seqs[2][10:]] + seqs[3:]
    body = "".join("%s %s\n" % (l, s) for l, s in zip(labels, bad))
    for interleaved in (False, True):
        assert _load(lib, tmp_path, "5 37\n" + body, interleaved) is None
        assert lib.errno == PLL_ERROR_PHYLIP_ILLEGALCHAR, lib.errmsg
        assert "'#'" in lib.errmsg and "line 4" in lib.errmsg, lib.errmsg


def test_phylip_missing_file(product_nogpu, tmp_path):
    lib = product_nogpu
    lib.errno = 0
    assert not lib.phylip_load(tmp_path / "nothing.phy")
    assert lib.errno == PLL_ERROR_FILE_OPEN


def test_msa_destroy_accepts_null(product_nogpu):
    product_nogpu.lib.pll_msa_destroy(None)


def test_reader_and_compression_symbols_are_exported(product_nogpu):
    names = """pll_fasta_open pll_fasta_getnext pll_fasta_close pll_fasta_rewind pll_phylip_load pll_msa_destroy
               pll_compress_site_patterns pll_compress_site_patterns_msa""".split()
    for n in names:
        assert hasattr(product_nogpu.lib, n), n
        assert n in pc.PLL_H_FUNCTIONS, n
    # the real readers, not the stubs the oracle keeps: a missing file is a file error, not "not implemented"
    product_nogpu.errno = 0
    assert not product_nogpu.fasta_open("/nonexistent/dir/x.fasta")
    assert product_nogpu.errno == PLL_ERROR_FILE_OPEN
