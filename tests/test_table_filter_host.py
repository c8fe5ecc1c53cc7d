"""The read-filter entries (pg_fastq_index, pg_table_read_hits, pg_fastq_gather: reads of a FASTQ text by their k-mers' counts in a
finished table, beside scripts/low_abd_reads.sh:10 / extract_unmapped.cpp) as far as the host decides about them: declared,
exported, mirrored in ``_lib``, every refusal returned BEFORE the first HIP call -- descriptors and buffers carry fake addresses
that are never dereferenced --, the argument handling of ``kmer_table filter``, and the reference the GPU tests compare with
(tests/_filter_ref.py) on an example whose answers are written out by hand.  No kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pangaea_amd import _lib, cli

from . import _filter_ref as ref
from .conftest import ROOT

OK, EINVAL = 0, -1
FAKE = 0x7F0000000000            # a 256-byte aligned address that belongs to nobody


def _table(kind=_lib.TABLE_MINI, k=21, log2_slots=20, log2_bucket_slots=10, data=FAKE):
    return _lib.pg_table(kind, k, log2_slots, log2_bucket_slots, data)


def _call(name, *args):
    L = _lib.load()
    rc = getattr(L, name)(*args)
    return rc, L.pg_last_error().decode()


def _define(hdr, name):
    m = re.search(r"#define\s+" + name + r"\s+(.+?)\s*(/\*|$)", hdr, flags=re.M)
    assert m, name
    return eval(m.group(1).replace("ull", "").replace("u", ""))


def test_header_declares_library_exports_and_lib_mirrors():
    hdr = open(os.path.join(ROOT, "include", "pangaea_feat.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+9\b", hdr) and _lib.ABI_VERSION == 9 and _lib.load().pg_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int64_t\s+pg_fastq_index_workspace_bytes\s*\(\s*int64_t n_bytes\s*\)", code)
    assert re.search(r"int\s+pg_fastq_index\s*\(\s*const uint8_t \*text,\s*int64_t n_bytes,\s*int64_t \*line_start\s*,\s*int64_t cap,\s*"
                     r"int64_t \*n_lines\s*,\s*void \*workspace,\s*int64_t workspace_bytes,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+pg_table_read_hits\s*\(\s*const pg_table \*t,\s*int k,\s*const uint8_t \*text,\s*int64_t n_bytes,\s*"
                     r"const int64_t \*line_start,\s*int64_t n_records,\s*int64_t first_record,\s*int64_t lower,\s*int64_t upper\s*,\s*"
                     r"int lowercase_is_base,\s*int min_qual_char\s*,\s*uint32_t \*hits\s*,\s*uint64_t \*status\s*,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+pg_fastq_gather\s*\(\s*const uint8_t \*text,\s*int64_t n_bytes,\s*const int64_t \*line_start,\s*int64_t n_records,\s*"
                     r"const int64_t \*kept,\s*const int64_t \*dst_off,\s*int64_t n_kept,\s*uint8_t \*out,\s*int64_t out_bytes,\s*void \*stream\s*\)", code)
    # each entry cites the step of the reference it stands beside
    for name in ("pg_fastq_index", "pg_table_read_hits", "pg_fastq_gather"):
        assert re.search(name + r"\s+beside scripts/low_abd_reads\.sh:10 / extract_unmapped\.cpp", hdr), name
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("pg_fastq_index_workspace_bytes", "pg_fastq_index", "pg_table_read_hits", "pg_fastq_gather"):
        assert hasattr(raw, name) and name in _lib.EXPORTS
    for name, mine in (("PG_STATUS_FASTQ_FORMAT", _lib.STATUS_FASTQ_FORMAT), ("PG_FASTQ_CLEAN", _lib.FASTQ_CLEAN), ("PG_FASTQ_NO_AT", _lib.FASTQ_NO_AT),
                       ("PG_FASTQ_NO_PLUS", _lib.FASTQ_NO_PLUS), ("PG_FASTQ_SHORT_QUALITY", _lib.FASTQ_SHORT_QUALITY),
                       ("PG_FASTQ_BAD_INDEX", _lib.FASTQ_BAD_INDEX)):
        assert _define(hdr, name) == mine, name
    # the new status bit is none of the old ones
    old = (_lib.STATUS_TABLE_FULL, _lib.STATUS_OVERFLOW_LIST, _lib.STATUS_PLAN_MISMATCH, _lib.STATUS_BOUNDS, _lib.STATUS_DEPTH_WORKSPACE)
    assert _lib.STATUS_FASTQ_FORMAT not in old and bin(_lib.STATUS_FASTQ_FORMAT).count("1") == 1


def test_index_workspace_bytes():
    L = _lib.load()
    assert L.pg_fastq_index_workspace_bytes(-1) == EINVAL
    # one count and one scanned count per tile of 4096 bytes, and the scan's last word
    assert L.pg_fastq_index_workspace_bytes(0) == 16
    assert L.pg_fastq_index_workspace_bytes(4096) == 32 and L.pg_fastq_index_workspace_bytes(4097) == 48
    assert L.pg_fastq_index_workspace_bytes(1 << 28) == (2 * (1 << 16) + 2) * 8


@pytest.mark.parametrize("args,text", [
    ((None, 100, FAKE, 64, FAKE, FAKE, 4096), "pg_fastq_index: text is null"),
    ((FAKE, -1, FAKE, 64, FAKE, FAKE, 4096), "pg_fastq_index: n_bytes is negative (-1)"),
    ((FAKE, 100, None, 64, FAKE, FAKE, 4096), "pg_fastq_index: line_start is null"),
    ((FAKE, 100, FAKE, 0, FAKE, FAKE, 4096), "pg_fastq_index: cap is below 1 (0)"),
    ((FAKE, 100, FAKE, 64, None, FAKE, 4096), "pg_fastq_index: n_lines is null"),
    ((FAKE + 8, 100, FAKE, 64, FAKE, FAKE, 4096), "pg_fastq_index: text is not 16-byte aligned"),
    ((FAKE, 100, FAKE, 64, FAKE, None, 4096), "pg_fastq_index: workspace of 4096 bytes, 32 needed (8-byte aligned)"),
    ((FAKE, 100, FAKE, 64, FAKE, FAKE + 4, 4096), "pg_fastq_index: workspace of 4096 bytes, 32 needed (8-byte aligned)"),
    ((FAKE, 100, FAKE, 64, FAKE, FAKE, 31), "pg_fastq_index: workspace of 31 bytes, 32 needed (8-byte aligned)"),
])
def test_index_refusals(args, text):
    rc, msg = _call("pg_fastq_index", *args, None)
    assert rc == EINVAL and msg == text


# (t, k, text, n_bytes, line_start, n_records, first_record, lower, upper, lowercase_is_base, min_qual_char, hits, status)
_GOOD = (_table(), 21, FAKE, 1000, FAKE, 4, 0, 1, -1, 1, 0, FAKE, FAKE)
_NAMES = ("t", "k", "text", "n_bytes", "line_start", "n_records", "first_record", "lower", "upper", "lowercase_is_base", "min_qual_char", "hits", "status")


def _with(**kw):
    assert set(kw) <= set(_NAMES)
    return tuple(kw.get(n, v) for n, v in zip(_NAMES, _GOOD))


@pytest.mark.parametrize("args,text", [
    (_with(t=None), "pg_table_read_hits: t is null"),
    (_with(text=None), "pg_table_read_hits: text is null"),
    (_with(line_start=None), "pg_table_read_hits: line_start is null"),
    (_with(hits=None), "pg_table_read_hits: hits is null"),
    (_with(status=None), "pg_table_read_hits: status is null"),
    (_with(n_bytes=-2), "pg_table_read_hits: n_bytes is negative (-2)"),
    (_with(n_records=-1), "pg_table_read_hits: n_records is negative (-1)"),
    (_with(first_record=-1), "pg_table_read_hits: first_record is negative (-1)"),
    (_with(lower=-1), "pg_table_read_hits: lower is negative (-1)"),
    (_with(lower=6, upper=5), "pg_table_read_hits: upper 5 is below lower 6"),
    (_with(lower=1, upper=0), "pg_table_read_hits: upper 0 is below lower 1"),
    (_with(min_qual_char=256), "pg_table_read_hits: min_qual_char 256 is no byte (0: none)"),
    (_with(min_qual_char=-1), "pg_table_read_hits: min_qual_char -1 is no byte (0: none)"),
    (_with(text=FAKE + 4), "pg_table_read_hits: text is not 16-byte aligned"),
    (_with(k=20), "pg_table_read_hits: k differs (table 21, asked 20)"),
    (_with(t=_table(kind=9)), "unknown table kind 9"),
    (_with(t=_table(k=12), k=12), "mini table needs 13 <= k <= 21 (got 12)"),
    (_with(t=_table(kind=_lib.TABLE_DENSE, k=17), k=17), "dense table needs 1 <= k <= 16 (got 17)"),
    (_with(t=_table(data=None)), "table descriptor is null"),
])
def test_read_hits_refusals(args, text):
    t = args[0]
    rc, msg = _call("pg_table_read_hits", None if t is None else C.byref(t), *args[1:], None)
    assert rc == EINVAL and msg == text


@pytest.mark.parametrize("args,text", [
    ((None, 100, FAKE, 4, FAKE, FAKE, 2, FAKE, 100), "pg_fastq_gather: text is null"),
    ((FAKE, 100, None, 4, FAKE, FAKE, 2, FAKE, 100), "pg_fastq_gather: line_start is null"),
    ((FAKE, -1, FAKE, 4, FAKE, FAKE, 2, FAKE, 100), "pg_fastq_gather: n_bytes is negative (-1)"),
    ((FAKE, 100, FAKE, -4, FAKE, FAKE, 0, FAKE, 100), "pg_fastq_gather: n_records is negative (-4)"),
    ((FAKE, 100, FAKE, 4, FAKE, FAKE, 5, FAKE, 100), "pg_fastq_gather: n_kept 5 outside [0, 4]"),
    ((FAKE, 100, FAKE, 4, FAKE, FAKE, -1, FAKE, 100), "pg_fastq_gather: n_kept -1 outside [0, 4]"),
    ((FAKE, 100, FAKE, 4, FAKE, FAKE, 2, FAKE, -1), "pg_fastq_gather: out_bytes is negative (-1)"),
    ((FAKE, 100, FAKE, 4, None, FAKE, 2, FAKE, 100), "pg_fastq_gather: kept or dst_off is null"),
    ((FAKE, 100, FAKE, 4, FAKE, None, 2, FAKE, 100), "pg_fastq_gather: kept or dst_off is null"),
    ((FAKE, 100, FAKE, 4, FAKE, FAKE, 2, None, 100), "pg_fastq_gather: out is null"),
])
def test_gather_refusals(args, text):
    rc, msg = _call("pg_fastq_gather", *args, None)
    assert rc == EINVAL and msg == text


def test_nothing_asked_is_ok_and_launches_nothing():
    assert _call("pg_fastq_index", FAKE, 0, FAKE, 1, FAKE, None, 0, None)[0] == OK
    for t in (_table(), _table(kind=_lib.TABLE_WIDE, k=31, log2_bucket_slots=0), _table(kind=_lib.TABLE_DENSE, k=4)):
        assert _call("pg_table_read_hits", C.byref(t), t.k, FAKE, 0, FAKE, 0, 0, 0, 0, 1, 0, FAKE, FAKE, None)[0] == OK
    assert _call("pg_fastq_gather", FAKE, 100, FAKE, 4, None, None, 0, None, 0, None)[0] == OK


# ------------------------------------------------------------------------------------------------------------ the tool

def _main(argv):
    try:
        return cli.main_kmer_table(argv)
    except SystemExit as e:
        return e.code


def _plan(argv):
    return cli._filter_plan(cli._kmer_table_parser().parse_args(["filter"] + argv))


def test_kmer_table_filter_arguments_accepted(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for name in ("a.fq", "b.fq", "t.fq", "u.fq", "t.dump"):
        (tmp_path / name).write_bytes(b"")
    src, reads, kw = _plan(["-k", "21", "-i", "a.fq", "-o", "out.fq"])
    assert src is None and reads == ("a.fq", None, "out.fq", None)
    assert kw == dict(lower=1, upper=None, min_hits=1, max_hits=None, pair="any", min_qual_char=None, lowercase_is_base=True)
    src, reads, kw = _plan(["-g", "t.dump", "-k", "15", "-1", "a.fq", "-2", "b.fq", "-o", "o1.fq", "-o2", "o2.fq", "-L", "0", "-U", "0",
                            "--min-hits", "0.5", "--max-hits", "1.0", "--pair", "both", "--min-qual-char", "?"])
    assert src == ("dump", "t.dump") and reads == ("a.fq", "b.fq", "o1.fq", "o2.fq")
    assert kw["lower"] == 0 and kw["upper"] == 0 and kw["min_hits"] == 0.5 and isinstance(kw["min_hits"], float)
    assert kw["max_hits"] == 1.0 and isinstance(kw["max_hits"], float) and kw["pair"] == "both" and kw["min_qual_char"] == "?"
    src, _, kw = _plan(["-ti", "t.fq", "-k", "31", "-i", "a.fq", "-o", "out.fq", "--pair", "single", "--min-hits", "3", "--max-hits", "40"])
    assert src == ("reads", "t.fq", None) and kw["min_hits"] == 3 and isinstance(kw["min_hits"], int) and kw["max_hits"] == 40
    src, _, _ = _plan(["-t1", "t.fq", "-t2", "u.fq", "-k", "21", "-i", "a.fq", "-o", "out.fq"])
    assert src == ("reads", "t.fq", "u.fq")
    monkeypatch.setenv("PANGAEA_LOWERCASE_IS_BASE", "0")
    assert _plan(["-k", "21", "-i", "a.fq", "-o", "out.fq"])[2]["lowercase_is_base"] is False
    assert sorted(os.listdir(tmp_path)) == ["a.fq", "b.fq", "t.dump", "t.fq", "u.fq"]


# (arguments, the reason ``_filter_plan`` gives -- a regular expression): each case is refused by one check of its own, by name
_REFUSED = [
    (["-k", "21", "-o", "out.fq"], r"the reads to filter are -i F or -1 F -2 F"),                                      # no reads
    (["-k", "40", "-i", "a.fq", "-o", "out.fq"], r"k-mer size 40 unsupported"),
    (["-k", "0", "-i", "a.fq", "-o", "out.fq"], r"k-mer size 0 unsupported"),
    (["-k", "21", "-i", "a.fq", "-1", "a.fq", "-2", "b.fq", "-o", "out.fq", "-o2", "o2.fq"], r"-i F or -1 F -2 F \(one of the two\)"),
    (["-k", "21", "-1", "a.fq", "-o", "out.fq"], r"-1 and -2 go together"),
    (["-k", "21", "-2", "b.fq", "-o", "out.fq"], r"-1 and -2 go together"),
    (["-k", "21", "-1", "a.fq", "-2", "b.fq", "-o", "out.fq"], r"writes two files: -o OUT -o2 OUT2"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "-o2", "o2.fq"], r"-o2 goes with -1 F -2 F"),
    (["-k", "21", "-g", "t.dump", "-ti", "t.fq", "-i", "a.fq", "-o", "out.fq"], r"the table from one source"),
    (["-k", "21", "-g", "t.dump", "-t1", "t.fq", "-t2", "t.fq", "-i", "a.fq", "-o", "out.fq"], r"the table from one source"),
    (["-k", "21", "-t1", "t.fq", "-i", "a.fq", "-o", "out.fq"], r"-t1 and -t2 go together"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "-L=-2"], r"-L must be at least 0 \(got -2\)"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "-L", "5", "-U", "4"], r"-U \(4\) is below -L \(5\)"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--min-hits", "1.5"], r"--min-hits 1\.5: a share lies in \[0, 1\]"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--min-hits=-1"], r"--min-hits -1: .*at least 0"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--max-hits", "2.0"], r"--max-hits 2\.0: a share lies in \[0, 1\]"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--min-hits", "half"], r"--min-hits takes a whole number or.*got 'half'"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--max-hits", "1e3"], r"--max-hits takes a whole number or.*got '1e3'"),
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
    (["-k", "x", "-i", "a.fq", "-o", "out.fq"], "argument -k/--kmer: invalid int value: 'x'"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "-L", "low"], "argument -L/--lower-count: invalid int value: 'low'"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--pairs", "any"], "unrecognized arguments: --pairs any"),
]


def _files(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for name in ("a.fq", "b.fq", "t.fq", "t.dump"):
        (tmp_path / name).write_bytes(b"")
    return ["a.fq", "b.fq", "t.dump", "t.fq"]


@pytest.mark.parametrize("argv,reason", _REFUSED, ids=[" ".join(a) for a, _ in _REFUSED])
def test_kmer_table_filter_refuses_for_the_reason(argv, reason, capsys, tmp_path, monkeypatch):
    """the check that refuses the arguments is the one named: ``_filter_plan`` raises it, before anything touches a device, and
    the tool ends with status 1 and that very message (on a machine without a GPU a call that got past the checks would end with
    status 1 too -- and another message)"""
    before = _files(tmp_path, monkeypatch)
    with pytest.raises(ValueError, match=reason):
        _plan(argv)
    assert _main(["filter"] + argv) == 1
    out = capsys.readouterr()
    assert out.out == "" and re.fullmatch(r"kmer_table: .*" + reason + r".*\n", out.err), out.err
    assert sorted(os.listdir(tmp_path)) == before


@pytest.mark.parametrize("argv,words", _UNPARSED, ids=[" ".join(a) for a, _ in _UNPARSED])
def test_kmer_table_filter_unparsed_arguments_exit_1(argv, words, capsys, tmp_path, monkeypatch):
    before = _files(tmp_path, monkeypatch)
    with pytest.raises(SystemExit) as e:
        cli._kmer_table_parser().parse_args(["filter"] + argv)
    assert e.value.code == 1
    assert words in capsys.readouterr().err
    assert _main(["filter"] + argv) == 1
    out = capsys.readouterr()
    assert out.out == "" and words in out.err and out.err.startswith("usage: kmer_table")
    assert sorted(os.listdir(tmp_path)) == before


def test_hit_bound_argument():
    for text, want in (("0", 0), ("1", 1), ("40", 40), ("0.0", 0.0), ("0.25", 0.25), ("1.0", 1.0), ("1.", 1.0), (".5", 0.5)):
        got = cli._hit_bound_arg(text, "--min-hits")
        assert got == want and type(got) is type(want)
    for text in ("1.5", "-1", "-0.5", "half", "", "1e3", "2.0"):
        with pytest.raises(ValueError, match="--max-hits"):
            cli._hit_bound_arg(text, "--max-hits")


# ------------------------------------------------------------------------------------------------------------ the reference

def _code(s: str) -> int:
    """canonical code of a k-mer string, by string operations alone: A0 C1 T2 G3, first character highest, the smaller strand"""
    rc = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    return min(int("".join(str("ACTG".index(c)) for c in x), 4) for x in (s, rc))


def _items(table: dict):
    pairs = sorted((_code(s), c) for s, c in table.items())
    return np.array([p[0] for p in pairs], np.uint64), np.array([p[1] for p in pairs], np.uint64)


SIX = (b"@r0\nACGT\n+\nIIII\n"            # ACG 5, CGT = rc(ACG) 5
       b"@r1 x\nAAAT\n+\nIIII\n"          # AAA 1, AAT 0
       b"@r2\nACNGG\n+r2\nIIIII\n"        # every 3-mer holds the N
       b"@r3\nacgGCC\n+\nII#III\n"        # acg 5, cgG 0, gGC 2, GCC = rc(GGC) 2
       b"@r4\nAC\n+\nII\n"                # shorter than k
       b"@r5\nGGCAAA\n+\nIIIIII")         # GGC 2, GCA 0, CAA 0, AAA 1; no final newline
TABLE = {"ACG": 5, "AAA": 1, "GGC": 2}


def test_reference_on_six_records_written_out_by_hand():
    assert _code("ACG") == 0 * 16 + 1 * 4 + 3 and _code("CGT") == _code("ACG") and _code("GCC") == _code("GGC") and _code("TTT") == 0
    items = _items(TABLE)
    recs = ref.records_of(SIX)
    assert len(recs) == 6 and [r[2] for r in recs] == [b"ACGT", b"AAAT", b"ACNGG", b"acgGCC", b"AC", b"GGCAAA"]
    assert SIX[recs[3][0]:recs[3][1]] == b"@r3\nacgGCC\n+\nII#III\n" and SIX[recs[5][0]:recs[5][1]] == b"@r5\nGGCAAA\n+\nIIIIII"
    # (n, h) under four windows
    assert ref.read_hits(SIX, 3, items, lower=2).tolist() == [[2, 2], [2, 0], [0, 0], [4, 3], [0, 0], [4, 1]]
    assert ref.read_hits(SIX, 3, items, lower=1).tolist() == [[2, 2], [2, 1], [0, 0], [4, 3], [0, 0], [4, 2]]
    assert ref.read_hits(SIX, 3, items, lower=0, upper=0).tolist() == [[2, 0], [2, 1], [0, 0], [4, 1], [0, 0], [4, 2]]
    assert ref.read_hits(SIX, 3, items, lower=2, upper=2).tolist() == [[2, 0], [2, 0], [0, 0], [4, 2], [0, 0], [4, 1]]
    # lower case is no base: r3 keeps GCC alone; a quality below '?' at its third base: the same
    assert ref.read_hits(SIX, 3, items, lower=2, lowercase_is_base=False).tolist() == [[2, 2], [2, 0], [0, 0], [1, 1], [0, 0], [4, 1]]
    assert ref.read_hits(SIX, 3, items, lower=2, min_qual_char="?").tolist() == [[2, 2], [2, 0], [0, 0], [1, 1], [0, 0], [4, 1]]
    # the selection: h >= half of n passes r0 and r3; at least one hit passes r5 too
    rec = [SIX[a:b] for a, b, _, _ in recs]
    half = dict(lower=2, min_hits=0.5)
    out, none, tot = ref.filter_fastq(SIX, 3, items, pair="single", **half)
    assert out == rec[0] + rec[3] and none is None
    assert tot == {"records": 6, "kept": 2, "passed": 2, "bases": 4 + 4 + 5 + 6 + 2 + 6, "kmers": 12, "hits": 6}
    assert ref.filter_fastq(SIX, 3, items, pair="any", **half)[0] == b"".join(rec[:4])
    assert ref.filter_fastq(SIX, 3, items, pair="both", **half)[0] == b""
    assert ref.filter_fastq(SIX, 3, items, pair="single", lower=2, min_hits=1)[0] == rec[0] + rec[3] + rec[5]
    assert ref.filter_fastq(SIX, 3, items, pair="any", lower=2, min_hits=1)[0] == SIX
    assert ref.filter_fastq(SIX, 3, items, pair="single", lower=2, min_hits=1, max_hits=0.5)[0] == rec[5]       # h <= n / 2: r0 (2 of 2), r3 (3 of 4) leave
    assert ref.filter_fastq(SIX, 3, items, pair="single", lower=2, min_hits=0, max_hits=0)[0] == rec[1]         # no hit at all, but a k-mer
    # R1 / R2: the first three records against the last three, mate by mate
    r1, r2 = b"".join(rec[:3]), b"".join(rec[3:])
    o1, o2, tot = ref.filter_fastq(r1, 3, items, r2, pair="any", **half)
    assert o1 == rec[0] and o2 == rec[3] and tot["records"] == 6 and tot["kept"] == 2 and tot["passed"] == 2
    assert ref.filter_fastq(r1, 3, items, r2, pair="both", **half)[:2] == (rec[0], rec[3])
    assert ref.filter_fastq(r1, 3, items, r2, pair="both", lower=2, min_hits=1)[:2] == (rec[0], rec[3])
    assert ref.filter_fastq(r1, 3, items, r2, pair="any", lower=2, min_hits=1)[:2] == (rec[0] + rec[2], rec[3] + rec[5])


def test_reference_names_the_first_malformed_record():
    items = _items(TABLE)
    for data, record in ((SIX[:SIX.index(b"+r2")], 2), (SIX.replace(b"@r1 x", b"r1 x"), 1), (SIX.replace(b"+r2", b"r2"), 2), (SIX + b"\n\n", 6),
                         (b"\n", 0)):
        with pytest.raises(ref.Malformed) as e:
            ref.filter_fastq(data, 3, items, pair="single")
        assert e.value.record == record
    with pytest.raises(ref.Malformed) as e:
        ref.read_hits(SIX.replace(b"II#III", b"II#II"), 3, items, min_qual_char="?")
    assert e.value.record == 3
    assert len(ref.read_hits(SIX.replace(b"II#III", b"II#II"), 3, items)) == 6          # without the threshold the quality line is not looked at
    with pytest.raises(ref.Malformed) as e:
        ref.filter_fastq(SIX[:SIX.index(b"@r5")], 3, items, pair="any")
    assert e.value.record == 4
    with pytest.raises(ref.Malformed):
        ref.filter_fastq(SIX, 3, items, SIX[:SIX.index(b"@r5")], pair="any")
    assert ref.records_of(b"") == [] and ref.filter_fastq(b"", 3, items)[0] == b""
