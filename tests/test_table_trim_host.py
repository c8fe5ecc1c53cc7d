"""The read-trimming entries (pg_table_read_spans, pg_fastq_gather_trimmed: reads of a FASTQ text cut to their solid k-mer span,
beside scripts/low_abd_reads.sh:10 / extract_unmapped.cpp) as far as the host decides about them: declared, exported, mirrored
in ``_lib``, every refusal returned BEFORE the first HIP call -- descriptors and buffers carry fake addresses that are never
dereferenced --, the argument handling of ``kmer_table trim``, and the reference the GPU tests compare with (tests/_trim_ref.py)
on examples whose answers are written out by hand.  No kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pangaea_amd import _lib, cli

from . import _trim_ref as ref
from .conftest import ROOT

OK, EINVAL = 0, -1
FAKE = 0x7F0000000000            # a 256-byte aligned address that belongs to nobody


def _table(kind=_lib.TABLE_MINI, k=21, log2_slots=20, log2_bucket_slots=10, data=FAKE):
    return _lib.pg_table(kind, k, log2_slots, log2_bucket_slots, data)


def _call(name, *args):
    L = _lib.load()
    rc = getattr(L, name)(*args)
    return rc, L.pg_last_error().decode()


def test_header_declares_library_exports_and_lib_mirrors():
    hdr = open(os.path.join(ROOT, "include", "pangaea_feat.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+9\b", hdr) and _lib.ABI_VERSION == 9 and _lib.load().pg_abi_version() == 9
    assert re.search(r"#define\s+PG_SPAN_FIRST\s+0\b", hdr) and _lib.SPAN_FIRST == 0
    assert re.search(r"#define\s+PG_SPAN_LONGEST\s+1\b", hdr) and _lib.SPAN_LONGEST == 1
    assert _lib.SPAN_MODES == {"first": 0, "longest": 1}
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+pg_table_read_spans\s*\(\s*const pg_table \*t,\s*int k,\s*const uint8_t \*text,\s*int64_t n_bytes,\s*"
                     r"const int64_t \*line_start,\s*int64_t n_records,\s*int64_t first_record,\s*int64_t lower,\s*int64_t upper\s*,\s*"
                     r"int lowercase_is_base,\s*int min_qual_char\s*,\s*int mode,\s*uint32_t \*spans\s*,\s*int64_t \*trimmed_bytes\s*,\s*"
                     r"uint64_t \*status\s*,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+pg_fastq_gather_trimmed\s*\(\s*const uint8_t \*text,\s*int64_t n_bytes,\s*const int64_t \*line_start,\s*int64_t n_records,\s*"
                     r"const int64_t \*kept,\s*const uint32_t \*spans\s*,\s*const int64_t \*dst_off,\s*int64_t n_kept,\s*uint8_t \*out,\s*"
                     r"int64_t out_bytes,\s*void \*stream\s*\)", code)
    # each entry cites the step of the reference it stands beside
    for name in ("pg_table_read_spans", "pg_fastq_gather_trimmed"):
        assert re.search(name + r"\s+beside scripts/low_abd_reads\.sh:10 / extract_unmapped\.cpp", hdr), name
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("pg_table_read_spans", "pg_fastq_gather_trimmed"):
        assert hasattr(raw, name) and name in _lib.EXPORTS


# (t, k, text, n_bytes, line_start, n_records, first_record, lower, upper, lowercase_is_base, min_qual_char, mode, spans, trimmed_bytes, status)
_GOOD = (_table(), 21, FAKE, 1000, FAKE, 4, 0, 1, -1, 1, 0, 1, FAKE, FAKE, FAKE)
_NAMES = ("t", "k", "text", "n_bytes", "line_start", "n_records", "first_record", "lower", "upper", "lowercase_is_base", "min_qual_char", "mode",
          "spans", "trimmed_bytes", "status")


def _with(**kw):
    assert set(kw) <= set(_NAMES)
    return tuple(kw.get(n, v) for n, v in zip(_NAMES, _GOOD))


@pytest.mark.parametrize("args,text", [
    (_with(t=None), "pg_table_read_spans: t is null"),
    (_with(text=None), "pg_table_read_spans: text is null"),
    (_with(line_start=None), "pg_table_read_spans: line_start is null"),
    (_with(spans=None), "pg_table_read_spans: spans is null"),
    (_with(trimmed_bytes=None), "pg_table_read_spans: trimmed_bytes is null"),
    (_with(status=None), "pg_table_read_spans: status is null"),
    (_with(n_bytes=-2), "pg_table_read_spans: n_bytes is negative (-2)"),
    (_with(n_records=-1), "pg_table_read_spans: n_records is negative (-1)"),
    (_with(first_record=-1), "pg_table_read_spans: first_record is negative (-1)"),
    (_with(lower=-1), "pg_table_read_spans: lower is negative (-1)"),
    (_with(lower=6, upper=5), "pg_table_read_spans: upper 5 is below lower 6"),
    (_with(lower=1, upper=0), "pg_table_read_spans: upper 0 is below lower 1"),
    (_with(min_qual_char=256), "pg_table_read_spans: min_qual_char 256 is no byte (0: none)"),
    (_with(min_qual_char=-1), "pg_table_read_spans: min_qual_char -1 is no byte (0: none)"),
    (_with(mode=2), "pg_table_read_spans: mode 2 is neither PG_SPAN_FIRST nor PG_SPAN_LONGEST"),
    (_with(mode=-1), "pg_table_read_spans: mode -1 is neither PG_SPAN_FIRST nor PG_SPAN_LONGEST"),
    (_with(text=FAKE + 4), "pg_table_read_spans: text is not 16-byte aligned"),
    (_with(k=20), "pg_table_read_spans: k differs (table 21, asked 20)"),
    (_with(t=_table(kind=9)), "unknown table kind 9"),
    (_with(t=_table(k=12), k=12), "mini table needs 13 <= k <= 21 (got 12)"),
    (_with(t=_table(kind=_lib.TABLE_DENSE, k=17), k=17), "dense table needs 1 <= k <= 16 (got 17)"),
    (_with(t=_table(data=None)), "table descriptor is null"),
])
def test_read_spans_refusals(args, text):
    t = args[0]
    rc, msg = _call("pg_table_read_spans", None if t is None else C.byref(t), *args[1:], None)
    assert rc == EINVAL and msg == text


# (text, n_bytes, line_start, n_records, kept, spans, dst_off, n_kept, out, out_bytes)
@pytest.mark.parametrize("args,text", [
    ((None, 100, FAKE, 4, FAKE, FAKE, FAKE, 2, FAKE, 100), "pg_fastq_gather_trimmed: text is null"),
    ((FAKE, 100, None, 4, FAKE, FAKE, FAKE, 2, FAKE, 100), "pg_fastq_gather_trimmed: line_start is null"),
    ((FAKE, -1, FAKE, 4, FAKE, FAKE, FAKE, 2, FAKE, 100), "pg_fastq_gather_trimmed: n_bytes is negative (-1)"),
    ((FAKE, 100, FAKE, -4, FAKE, FAKE, FAKE, 0, FAKE, 100), "pg_fastq_gather_trimmed: n_records is negative (-4)"),
    ((FAKE, 100, FAKE, 4, FAKE, FAKE, FAKE, 5, FAKE, 100), "pg_fastq_gather_trimmed: n_kept 5 outside [0, 4]"),
    ((FAKE, 100, FAKE, 4, FAKE, FAKE, FAKE, -1, FAKE, 100), "pg_fastq_gather_trimmed: n_kept -1 outside [0, 4]"),
    ((FAKE, 100, FAKE, 4, FAKE, FAKE, FAKE, 2, FAKE, -1), "pg_fastq_gather_trimmed: out_bytes is negative (-1)"),
    ((FAKE, 100, FAKE, 4, None, FAKE, FAKE, 2, FAKE, 100), "pg_fastq_gather_trimmed: kept is null"),
    ((FAKE, 100, FAKE, 4, FAKE, None, FAKE, 2, FAKE, 100), "pg_fastq_gather_trimmed: spans is null"),
    ((FAKE, 100, FAKE, 4, FAKE, FAKE, None, 2, FAKE, 100), "pg_fastq_gather_trimmed: dst_off is null"),
    ((FAKE, 100, FAKE, 4, FAKE, FAKE, FAKE, 2, None, 100), "pg_fastq_gather_trimmed: out is null"),
])
def test_gather_trimmed_refusals(args, text):
    rc, msg = _call("pg_fastq_gather_trimmed", *args, None)
    assert rc == EINVAL and msg == text


def test_nothing_asked_is_ok_and_launches_nothing():
    for t in (_table(), _table(kind=_lib.TABLE_WIDE, k=31, log2_bucket_slots=0), _table(kind=_lib.TABLE_DENSE, k=4)):
        for mode in (_lib.SPAN_FIRST, _lib.SPAN_LONGEST):
            assert _call("pg_table_read_spans", C.byref(t), t.k, FAKE, 0, FAKE, 0, 0, 0, 0, 1, 0, mode, FAKE, FAKE, FAKE, None)[0] == OK
    assert _call("pg_fastq_gather_trimmed", FAKE, 100, FAKE, 4, None, None, None, 0, None, 0, None)[0] == OK


# ------------------------------------------------------------------------------------------------------------ the tool

def _main(argv):
    try:
        return cli.main_kmer_table(argv)
    except SystemExit as e:
        return e.code


def _plan(argv):
    return cli._trim_plan(cli._kmer_table_parser().parse_args(["trim"] + argv))


def test_kmer_table_trim_arguments_accepted(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for name in ("a.fq", "b.fq", "t.fq", "u.fq", "t.dump"):
        (tmp_path / name).write_bytes(b"")
    src, reads, kw = _plan(["-k", "21", "-i", "a.fq", "-o", "out.fq"])
    assert src is None and reads == ("a.fq", None, "out.fq", None)
    assert kw == dict(lower=1, upper=None, mode="longest", min_len=None, pair="both", min_qual_char=None, lowercase_is_base=True)
    src, reads, kw = _plan(["-g", "t.dump", "-k", "15", "-1", "a.fq", "-2", "b.fq", "-o", "o1.fq", "-o2", "o2.fq", "-L", "2", "-U", "9",
                            "--mode", "first", "--min-len", "50", "--pair", "any", "--min-qual-char", "?"])
    assert src == ("dump", "t.dump") and reads == ("a.fq", "b.fq", "o1.fq", "o2.fq")
    assert kw == dict(lower=2, upper=9, mode="first", min_len=50, pair="any", min_qual_char="?", lowercase_is_base=True)
    src, _, kw = _plan(["-ti", "t.fq", "-k", "31", "-i", "a.fq", "-o", "out.fq", "--pair", "single", "--min-len", "1"])
    assert src == ("reads", "t.fq", None) and kw["min_len"] == 1 and kw["pair"] == "single"
    src, _, _ = _plan(["-t1", "t.fq", "-t2", "u.fq", "-k", "21", "-i", "a.fq", "-o", "out.fq"])
    assert src == ("reads", "t.fq", "u.fq")
    monkeypatch.setenv("PANGAEA_LOWERCASE_IS_BASE", "0")
    assert _plan(["-k", "21", "-i", "a.fq", "-o", "out.fq"])[2]["lowercase_is_base"] is False
    assert sorted(os.listdir(tmp_path)) == ["a.fq", "b.fq", "t.dump", "t.fq", "u.fq"]


# (arguments, the reason ``_trim_plan`` gives -- a regular expression): each case is refused by one check of its own, by name
_REFUSED = [
    (["-k", "21", "-o", "out.fq"], r"the reads to trim are -i F or -1 F -2 F"),                                        # no reads
    (["-k", "40", "-i", "a.fq", "-o", "out.fq"], r"k-mer size 40 unsupported"),
    (["-k", "0", "-i", "a.fq", "-o", "out.fq"], r"k-mer size 0 unsupported"),
    (["-k", "21", "-i", "a.fq", "-1", "a.fq", "-2", "b.fq", "-o", "out.fq", "-o2", "o2.fq"], r"-i F or -1 F -2 F \(one of the two\)"),
    (["-k", "21", "-1", "a.fq", "-o", "out.fq"], r"-1 and -2 go together"),
    (["-k", "21", "-2", "b.fq", "-o", "out.fq"], r"-1 and -2 go together"),
    (["-k", "21", "-1", "a.fq", "-2", "b.fq", "-o", "out.fq"], r"writes two files: -o OUT -o2 OUT2"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "-o2", "o2.fq"], r"-o2 goes with -1 F -2 F"),
    (["-k", "21", "-g", "t.dump", "-ti", "t.fq", "-i", "a.fq", "-o", "out.fq"], r"trim takes the table from one source"),
    (["-k", "21", "-g", "t.dump", "-t1", "t.fq", "-t2", "t.fq", "-i", "a.fq", "-o", "out.fq"], r"trim takes the table from one source"),
    (["-k", "21", "-t1", "t.fq", "-i", "a.fq", "-o", "out.fq"], r"-t1 and -t2 go together"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "-L=-2"], r"-L must be at least 0 \(got -2\)"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "-L", "5", "-U", "4"], r"-U \(4\) is below -L \(5\)"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--mode", "last"], r"--mode must be first or longest \(got 'last'\)"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--min-len", "0"], r"--min-len must be at least 1 \(got 0\)"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--min-len=-5"], r"--min-len must be at least 1 \(got -5\)"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--pair", "all"], r"--pair must be any, both or single \(got 'all'\)"),
    (["-k", "21", "-1", "a.fq", "-2", "b.fq", "-o", "out.fq", "-o2", "o2.fq", "--pair", "single"], r"--pair single judges the records of one file"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--min-qual-char", "??"], r"--min-qual-char takes one character \(got '\?\?'\)"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq.gz"], r"out\.fq\.gz: the kept reads are written as plain text"),
    (["-k", "21", "-1", "a.fq", "-2", "b.fq", "-o", "out.fq", "-o2", "o2.fq.gz"], r"o2\.fq\.gz: the kept reads are written as plain text"),
    (["-k", "21", "-i", "not_there.fq", "-o", "out.fq"], r"not_there\.fq: no such file"),
    (["-k", "21", "-1", "a.fq", "-2", "not_there.fq", "-o", "out.fq", "-o2", "o2.fq"], r"not_there\.fq: no such file"),
    (["-k", "21", "-g", "not_there.dump", "-i", "a.fq", "-o", "out.fq"], r"not_there\.dump: no such file"),
    (["-k", "21", "-t1", "t.fq", "-t2", "not_there.fq", "-i", "a.fq", "-o", "out.fq"], r"not_there\.fq: no such file"),
]
# what the argument parser itself refuses, and the words of its message
_UNPARSED = [
    (["-k", "21", "-i", "a.fq"], "the following arguments are required: -o/--output"),
    (["-i", "a.fq", "-o", "out.fq"], "the following arguments are required: -k/--kmer"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--min-len", "long"], "argument --min-len: invalid int value: 'long'"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--min-hits", "3"], "unrecognized arguments: --min-hits 3"),
]


def _files(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for name in ("a.fq", "b.fq", "t.fq", "t.dump"):
        (tmp_path / name).write_bytes(b"")
    return ["a.fq", "b.fq", "t.dump", "t.fq"]


@pytest.mark.parametrize("argv,reason", _REFUSED, ids=[" ".join(a) for a, _ in _REFUSED])
def test_kmer_table_trim_refuses_for_the_reason(argv, reason, capsys, tmp_path, monkeypatch):
    """the check that refuses the arguments is the one named: ``_trim_plan`` raises it, before anything touches a device, and the
    tool ends with status 1 and that very message"""
    before = _files(tmp_path, monkeypatch)
    with pytest.raises(ValueError, match=reason):
        _plan(argv)
    assert _main(["trim"] + argv) == 1
    out = capsys.readouterr()
    assert out.out == "" and re.fullmatch(r"kmer_table: .*" + reason + r".*\n", out.err), out.err
    assert sorted(os.listdir(tmp_path)) == before


@pytest.mark.parametrize("argv,words", _UNPARSED, ids=[" ".join(a) for a, _ in _UNPARSED])
def test_kmer_table_trim_unparsed_arguments_exit_1(argv, words, capsys, tmp_path, monkeypatch):
    before = _files(tmp_path, monkeypatch)
    assert _main(["trim"] + argv) == 1
    out = capsys.readouterr()
    assert out.out == "" and words in out.err and out.err.startswith("usage: kmer_table")
    assert sorted(os.listdir(tmp_path)) == before


# ------------------------------------------------------------------------------------------------------------ the reference

def _code(s: str) -> int:
    """canonical code of a k-mer string, by string operations alone: A0 C1 T2 G3, first character highest, the smaller strand"""
    rc = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    return min(int("".join(str("ACTG".index(c)) for c in x), 4) for x in (s, rc))


def _items(table: dict):
    pairs = sorted((_code(s), c) for s, c in table.items())
    return np.array([p[0] for p in pairs], np.uint64), np.array([p[1] for p in pairs], np.int64)


# k = 3.  The made-up table: ACG (= CGT) 5, CGA (= TCG) 5, GAC (= GTC) 5, AAC (= GTT) 2, ACA (= TGT) 2, CAA (= TTG) 9
TABLE = {"ACG": 5, "CGA": 5, "GAC": 5, "AAC": 2, "ACA": 2, "CAA": 9}


def _rec(name: bytes, seq: bytes, qual: bytes = None, eol: bytes = b"\n", last: bytes = None) -> bytes:
    qual = b"I" * len(seq) if qual is None else qual
    return b"@" + name + eol + seq + eol + b"+" + eol + qual + (eol if last is None else last)


def test_runs_and_spans_of_flag_vectors():
    f = lambda s: np.array([c == "1" for c in s])       # noqa: E731
    assert ref.runs_of(f("")) == [] and ref.runs_of(f("000")) == [] and ref.runs_of(f("111")) == [(0, 3)]
    assert ref.runs_of(f("0110111001")) == [(1, 3), (4, 7), (9, 10)]
    assert ref.span_of(f("0110111001"), 5, "longest") == (4, 3 + 4) and ref.span_of(f("0110111001"), 5, "first") == (0, 0)
    assert ref.span_of(f("1101100"), 3, "longest") == (0, 4) and ref.span_of(f("1101100"), 3, "first") == (0, 4)        # equal runs: the leftmost
    assert ref.span_of(f("1011"), 3, "longest") == (2, 4) and ref.span_of(f("1011"), 3, "first") == (0, 3)              # a later longer run
    assert ref.span_of(f("000"), 3, "longest") == (0, 0) and ref.span_of(f(""), 3, "first") == (0, 0)
    assert ref.span_of(f("1"), 7, "longest") == (0, 7)


def test_reference_on_records_written_out_by_hand():
    items = _items(TABLE)
    assert _code("CGT") == _code("ACG") and _code("TCG") == _code("CGA") and _code("GTC") == _code("GAC")
    k = 3

    def rows(data, **kw):
        return ref.read_spans(data, k, items, **kw).tolist()

    # one run: ACGAC -> ACG CGA GAC, all 5; then ACT 0 ... : positions 0 1 2 solid, 3 4 not
    one = _rec(b"one", b"ACGACTT")                      # ACG CGA GAC ACT CTT
    assert rows(one) == [[5, 3, 0, 5]] and rows(one, mode="first") == [[5, 3, 0, 5]]
    assert ref.trim_fastq(one, k, items, pair="single")[0] == b"@one\nACGAC\n+\nIIIII\n"
    # two equal runs, the leftmost wins: ACGA T ACGA: ACG CGA GAT ATA TAC ACG CGA -> 1 1 0 0 0 1 1: runs [0, 2) and [5, 7)
    two = _rec(b"two", b"ACGATACGA", b"ABCDEFGHI")
    assert rows(two) == [[7, 4, 0, 4]] and rows(two, mode="first") == [[7, 4, 0, 4]]
    assert ref.trim_fastq(two, k, items, pair="single")[0] == b"@two\nACGA\n+\nABCD\n"
    # a later longer run: ACG T ACGAC: ACG CGT GTA TAC ACG CGA GAC -> 1 1 0 0 1 1 1 (CGT = ACG): [0, 2) and [4, 7)
    later = _rec(b"later", b"ACGTACGAC", b"ABCDEFGHI")
    assert rows(later) == [[7, 5, 4, 5]] and rows(later, mode="first") == [[7, 5, 0, 4]]
    assert ref.trim_fastq(later, k, items, pair="single")[0] == b"@later\nACGAC\n+\nEFGHI\n"
    assert ref.trim_fastq(later, k, items, pair="single", mode="first")[0] == b"@later\nACGT\n+\nABCD\n"
    # position 0 not solid under `first`: TACGAC: TAC ACG CGA GAC -> 0 1 1 1
    late = _rec(b"late", b"TACGAC")
    assert rows(late) == [[4, 3, 1, 5]] and rows(late, mode="first") == [[4, 3, 0, 0]]
    out, _, tot = ref.trim_fastq(late, k, items, pair="single", mode="first")
    assert out == b"" and tot == {"records": 1, "kept": 0, "passed": 0, "trimmed": 0, "bases": 6, "bases_out": 0, "kmers": 4, "hits": 3}
    # the window: counts 2 .. 5 leave CAA (9) out: AACAAC: AAC ACA CAA AAC -> 1 1 0 1; an N holds no k-mer: ACGNCGA -> ACG . . . CGA
    win = _rec(b"win", b"AACAAC") + _rec(b"n", b"ACGNCGA")
    assert rows(win, lower=2, upper=5) == [[4, 3, 0, 4], [2, 2, 0, 3]] and rows(win) == [[4, 4, 0, 6], [2, 2, 0, 3]]
    assert rows(win, lower=0, upper=0) == [[4, 0, 0, 0], [2, 0, 0, 0]]
    # CRLF: the '\r' is a byte of the line, holds no k-mer, and stays at the end of both cut lines
    crlf = _rec(b"crlf", b"TACGACT", b"ABCDEFG", eol=b"\r\n")
    assert rows(crlf) == [[5, 3, 1, 5]]                 # TAC ACG CGA GAC ACT; "CT\r" holds none
    assert ref.trim_fastq(crlf, k, items, pair="single")[0] == b"@crlf\r\nACGAC\r\n+\r\nBCDEF\r\n"
    # a sequence line with '\r' beside a quality line without: each keeps what it had
    mixed = b"@m\nTACGAC\r\n+\nABCDEF\n"
    assert ref.trim_fastq(mixed, k, items, pair="single")[0] == b"@m\nACGAC\r\n+\nBCDEF\n"
    # long quality: what lies beyond the sequence is dropped
    longq = _rec(b"long", b"ACGAC", b"ABCDEFGH")
    out, _, tot = ref.trim_fastq(longq, k, items, pair="single")
    assert out == b"@long\nACGAC\n+\nABCDE\n" and tot["trimmed"] == 1 and tot["bases"] == 5 and tot["bases_out"] == 5
    # no final newline: the last record leaves without one; the one in front keeps its own
    nonl = _rec(b"a", b"TACGAC") + _rec(b"b", b"ACGACTT", b"ABCDEFG", last=b"")
    out, _, tot = ref.trim_fastq(nonl, k, items, pair="both")
    assert out == b"@a\nACGAC\n+\nIIIII\n@b\nACGAC\n+\nABCDE"
    assert tot == {"records": 2, "kept": 2, "passed": 2, "trimmed": 2, "bases": 13, "bases_out": 10, "kmers": 9, "hits": 6}
    # untrimmed records are not counted as trimmed; min_len and the pair rules
    whole = _rec(b"w", b"ACGAC") + _rec(b"s", b"TTACGTT")       # TTA TAC ACG CGT GTT -> 0 0 1 1 1 (GTT = AAC): span (2, 5)
    assert rows(whole) == [[3, 3, 0, 5], [5, 3, 2, 5]]
    out, _, tot = ref.trim_fastq(whole, k, items, pair="both")
    assert out == _rec(b"w", b"ACGAC") + b"@s\nACGTT\n+\nIIIII\n" and tot["trimmed"] == 1 and tot["kept"] == 2
    pairs = _rec(b"p1", b"ACGAC") + _rec(b"p2", b"TTTTT")       # p2 has no solid position
    assert ref.trim_fastq(pairs, k, items, pair="both")[0] == b""
    out, _, tot = ref.trim_fastq(pairs, k, items, pair="any")
    assert out == _rec(b"p1", b"ACGAC") + b"@p2\n\n+\n\n" and tot["kept"] == 2 and tot["passed"] == 1 and tot["trimmed"] == 1
    assert ref.trim_fastq(pairs, k, items, pair="single")[0] == _rec(b"p1", b"ACGAC")
    assert ref.trim_fastq(pairs, k, items, pair="single", min_len=6)[0] == b""
    o1, o2, tot = ref.trim_fastq(_rec(b"p1", b"ACGAC"), k, items, _rec(b"p2", b"TACGT"), pair="both", min_len=4)
    assert o1 == _rec(b"p1", b"ACGAC") and o2 == b"@p2\nACGT\n+\nIIII\n" and tot["records"] == 2 and tot["trimmed"] == 1
    # lower case and the quality threshold mask bases: without the 'a' CGA and GAC stay; a '#' under the middle base leaves none
    low = _rec(b"low", b"aCGAC", b"II#II")
    assert rows(low) == [[3, 3, 0, 5]] and rows(low, lowercase_is_base=False) == [[2, 2, 1, 4]]
    assert rows(low, min_qual_char="?") == [[0, 0, 0, 0]]        # every 3-mer of five bases holds the masked third one


def test_reference_names_the_first_malformed_record():
    items = _items(TABLE)
    good = _rec(b"g", b"ACGAC")
    for data, record in ((good + b"@x\nACG\n+\n", 1), (good + good.replace(b"@", b"", 1), 1), (good.replace(b"+", b"-"), 0), (good + b"\n", 1),
                         (b"\n", 0), (good + _rec(b"short", b"ACGAC", b"IIII"), 1), (good + b"@s\nACGAC\r\n+\nIIII\r\n", 1)):
        with pytest.raises(ref.Malformed) as e:
            ref.trim_fastq(data, 3, items, pair="single")
        assert e.value.record == record
    # a quality line without the '\r' its sequence line has is as long as it need be -- unless a threshold compares them byte by byte
    mixed = b"@m\nTACGAC\r\n+\nABCDEF\n"
    assert len(ref.read_spans(mixed, 3, items)) == 1
    with pytest.raises(ref.Malformed):
        ref.read_spans(mixed, 3, items, min_qual_char="?")
    with pytest.raises(ref.Malformed) as e:
        ref.trim_fastq(good * 3, 3, items, pair="both")
    assert e.value.record == 2
    with pytest.raises(ref.Malformed):
        ref.trim_fastq(good * 2, 3, items, good, pair="any")
    assert ref.records_of(b"") == [] and ref.trim_fastq(b"", 3, items)[0] == b""
