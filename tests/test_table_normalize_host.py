"""The read-depth entry (pg_table_read_depths: an order statistic of the k-mer counts of every record of a FASTQ text and the draw of
its unit, beside scripts/low_abd_reads.sh:10 / extract_unmapped.cpp) as far as the host decides about it: declared, exported,
mirrored in ``_lib``, every refusal returned BEFORE the first HIP call -- descriptors and buffers carry fake addresses that are
never dereferenced --, the argument handling of ``kmer_table normalize``, the draw's known answers, and the reference the GPU
tests compare with (tests/_normalize_ref.py) on an example whose rows and kept records are written out by hand.  No kernel is
launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pangaea_amd import _lib, cli

from . import _normalize_ref as ref
from .conftest import ROOT

OK, EINVAL = 0, -1
FAKE = 0x7F0000000000            # a 256-byte aligned address that belongs to nobody
WHO = "pg_table_read_depths"


def _table(kind=_lib.TABLE_MINI, k=21, log2_slots=20, log2_bucket_slots=10, data=FAKE):
    return _lib.pg_table(kind, k, log2_slots, log2_bucket_slots, data)


def _call(name, *args):
    L = _lib.load()
    rc = getattr(L, name)(*args)
    return rc, L.pg_last_error().decode()


def test_header_declares_library_exports_and_lib_mirrors():
    hdr = open(os.path.join(ROOT, "include", "pangaea_feat.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+9\b", hdr) and _lib.ABI_VERSION == 9 and _lib.load().pg_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+pg_table_read_depths\s*\(\s*const pg_table \*t,\s*int k,\s*const uint8_t \*text,\s*int64_t n_bytes,\s*"
                     r"const int64_t \*line_start,\s*int64_t n_records,\s*int64_t first_record,\s*int64_t lower\s*,\s*int percentile\s*,\s*"
                     r"int lowercase_is_base,\s*int min_qual_char\s*,\s*uint64_t seed,\s*int unit_log2\s*,\s*uint32_t \*rows\s*,\s*"
                     r"uint64_t \*status\s*,\s*void \*stream\s*\)", code)
    assert re.search(WHO + r"\s+beside scripts/low_abd_reads\.sh:10 / extract_unmapped\.cpp", hdr)
    assert "Depth of the reads of a FASTQ text" in hdr
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, WHO) and WHO in _lib.EXPORTS
    assert _lib.load().pg_table_read_depths.argtypes is not None and len(_lib.load().pg_table_read_depths.argtypes) == 16


_NAMES = ("t", "k", "text", "n_bytes", "line_start", "n_records", "first_record", "lower", "percentile", "lowercase_is_base", "min_qual_char",
          "seed", "unit_log2", "rows", "status")
_GOOD = (_table(), 21, FAKE, 1000, FAKE, 4, 0, 1, 50, 1, 0, 7, 1, FAKE, FAKE)


def _with(**kw):
    assert set(kw) <= set(_NAMES)
    return tuple(kw.get(n, v) for n, v in zip(_NAMES, _GOOD))


@pytest.mark.parametrize("args,text", [
    (_with(t=None), WHO + ": t is null"),
    (_with(text=None), WHO + ": text is null"),
    (_with(line_start=None), WHO + ": line_start is null"),
    (_with(rows=None), WHO + ": rows is null"),
    (_with(status=None), WHO + ": status is null"),
    (_with(n_bytes=-2), WHO + ": n_bytes is negative (-2)"),
    (_with(n_records=-1), WHO + ": n_records is negative (-1)"),
    (_with(first_record=-1), WHO + ": first_record is negative (-1)"),
    (_with(lower=0), WHO + ": lower is below 1 (0)"),
    (_with(lower=-3), WHO + ": lower is below 1 (-3)"),
    (_with(percentile=-1), WHO + ": percentile -1 outside [0, 100]"),
    (_with(percentile=101), WHO + ": percentile 101 outside [0, 100]"),
    (_with(min_qual_char=256), WHO + ": min_qual_char 256 is no byte (0: none)"),
    (_with(min_qual_char=-1), WHO + ": min_qual_char -1 is no byte (0: none)"),
    (_with(unit_log2=2), WHO + ": unit_log2 2 is neither 0 nor 1"),
    (_with(unit_log2=-1), WHO + ": unit_log2 -1 is neither 0 nor 1"),
    (_with(text=FAKE + 4), WHO + ": text is not 16-byte aligned"),
    (_with(rows=FAKE + 8), WHO + ": rows is not 16-byte aligned"),
    (_with(k=20), WHO + ": k differs (table 21, asked 20)"),
    (_with(t=_table(kind=9)), "unknown table kind 9"),
    (_with(t=_table(k=12), k=12), "mini table needs 13 <= k <= 21 (got 12)"),
    (_with(t=_table(kind=_lib.TABLE_DENSE, k=17), k=17), "dense table needs 1 <= k <= 16 (got 17)"),
    (_with(t=_table(data=None)), "table descriptor is null"),
])
def test_read_depths_refusals(args, text):
    t = args[0]
    rc, msg = _call(WHO, None if t is None else C.byref(t), *args[1:], None)
    assert rc == EINVAL and msg == text


def test_nothing_asked_is_ok_and_launches_nothing():
    for t in (_table(), _table(kind=_lib.TABLE_WIDE, k=31, log2_bucket_slots=0), _table(kind=_lib.TABLE_DENSE, k=4)):
        for percentile, unit_log2, seed in ((0, 0, 0), (100, 1, (1 << 64) - 1)):
            assert _call(WHO, C.byref(t), t.k, FAKE, 0, FAKE, 0, 0, 1, percentile, 1, 0, seed, unit_log2, FAKE, FAKE, None)[0] == OK


# ------------------------------------------------------------------------------------------------------------ the tool

def _main(argv):
    try:
        return cli.main_kmer_table(argv)
    except SystemExit as e:
        return e.code


def _plan(argv):
    return cli._normalize_plan(cli._kmer_table_parser().parse_args(["normalize"] + argv))


def test_kmer_table_normalize_arguments_accepted(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for name in ("a.fq", "b.fq", "t.fq", "u.fq", "t.dump"):
        (tmp_path / name).write_bytes(b"")
    src, reads, kw = _plan(["-k", "21", "-i", "a.fq", "--target", "20", "-o", "out.fq"])
    assert src is None and reads == ("a.fq", None, "out.fq", None)
    assert kw == dict(target=20, min_depth=0, lower=1, percentile=50, pair="any", seed=0, min_qual_char=None, lowercase_is_base=True)
    src, reads, kw = _plan(["-g", "t.dump", "-k", "15", "-1", "a.fq", "-2", "b.fq", "-o", "o1.fq", "-o2", "o2.fq", "-L", "2", "--target", "2147483647",
                            "--min-depth", "3", "--percentile", "0", "--pair", "both", "--seed", "18446744073709551615", "--min-qual-char", "?"])
    assert src == ("dump", "t.dump") and reads == ("a.fq", "b.fq", "o1.fq", "o2.fq")
    assert kw == dict(target=(1 << 31) - 1, min_depth=3, lower=2, percentile=0, pair="both", seed=(1 << 64) - 1, min_qual_char="?",
                      lowercase_is_base=True)
    src, _, kw = _plan(["-ti", "t.fq", "-k", "31", "-i", "a.fq", "--target", "1", "--percentile", "100", "--pair", "single", "-o", "out.fq"])
    assert src == ("reads", "t.fq", None) and kw["pair"] == "single" and kw["percentile"] == 100 and kw["target"] == 1
    src, _, _ = _plan(["-t1", "t.fq", "-t2", "u.fq", "-k", "21", "-i", "a.fq", "--target", "5", "-o", "out.fq"])
    assert src == ("reads", "t.fq", "u.fq")
    monkeypatch.setenv("PANGAEA_LOWERCASE_IS_BASE", "0")
    assert _plan(["-k", "21", "-i", "a.fq", "--target", "5", "-o", "out.fq"])[2]["lowercase_is_base"] is False
    assert sorted(os.listdir(tmp_path)) == ["a.fq", "b.fq", "t.dump", "t.fq", "u.fq"]


def test_kmer_table_normalize_help_says_what_it_does(capsys):
    assert _main(["normalize", "--help"]) == 0
    out = " ".join(capsys.readouterr().out.split())
    assert "target / depth" in out and "the usual call" in out
    assert "kmer_table normalize" in cli.__doc__ and "``kmer_table normalize``" in cli.main_kmer_table.__doc__


_BASE = ["-k", "21", "-i", "a.fq", "-o", "out.fq"]
# (arguments, the reason ``_normalize_plan`` gives -- a regular expression)
_REFUSED = [
    (_BASE, r"--target is the depth to normalise to, a whole number of at least 1 \(got None\)"),
    (_BASE + ["--target", "0"], r"--target is the depth to normalise to, a whole number of at least 1 \(got 0\)"),
    (_BASE + ["--target=-4"], r"--target is the depth to normalise to, a whole number of at least 1 \(got -4\)"),
    (_BASE + ["--target", "2147483648"], r"--target must be below 2\^31 \(got 2147483648\)"),
    (_BASE + ["--target", "8", "--min-depth=-1"], r"--min-depth must be at least 0 \(got -1\)"),
    (_BASE + ["--target", "8", "--percentile", "101"], r"--percentile must lie in 0\.\.100 \(got 101\)"),
    (_BASE + ["--target", "8", "--percentile=-1"], r"--percentile must lie in 0\.\.100 \(got -1\)"),
    (_BASE + ["--target", "8", "--seed", "18446744073709551616"], r"--seed must lie in \[0, 2\^64\) \(got 18446744073709551616\)"),
    (_BASE + ["--target", "8", "--seed=-1"], r"--seed must lie in \[0, 2\^64\) \(got -1\)"),
    (_BASE + ["--target", "8", "-L", "0"], r"-L must be at least 1 \(got 0\)"),
    (_BASE + ["--target", "8", "-L=-2"], r"-L must be at least 0 \(got -2\)"),                                          # (the shared check comes first)
    (["-k", "21", "--target", "8", "-o", "out.fq"], r"the reads to normalize are -i F or -1 F -2 F"),
    (["-k", "40", "-i", "a.fq", "--target", "8", "-o", "out.fq"], r"k-mer size 40 unsupported"),
    (["-k", "21", "-1", "a.fq", "--target", "8", "-o", "out.fq"], r"-1 and -2 go together"),
    (["-k", "21", "-1", "a.fq", "-2", "b.fq", "--target", "8", "-o", "out.fq"], r"writes two files: -o OUT -o2 OUT2"),
    (_BASE + ["--target", "8", "-o2", "o2.fq"], r"-o2 goes with -1 F -2 F"),
    (_BASE + ["--target", "8", "-g", "t.dump", "-ti", "t.fq"], r"normalize takes the table from one source"),
    (_BASE + ["--target", "8", "--pair", "some"], r"--pair must be any, both or single \(got 'some'\)"),
    (["-k", "21", "-1", "a.fq", "-2", "b.fq", "--target", "8", "--pair", "single", "-o", "o.fq", "-o2", "o2.fq"], r"--pair single judges the records of one file"),
    (_BASE + ["--target", "8", "--min-qual-char", "??"], r"--min-qual-char takes one character \(got '\?\?'\)"),
    (["-k", "21", "-i", "a.fq", "--target", "8", "-o", "out.fq.gz"], r"out\.fq\.gz: the kept reads are written as plain text"),
    (["-k", "21", "-i", "not_there.fq", "--target", "8", "-o", "out.fq"], r"not_there\.fq: no such file"),
    (_BASE + ["--target", "8", "-g", "not_there.dump"], r"not_there\.dump: no such file"),
]
# what the argument parser itself refuses, and the words of its message
_UNPARSED = [
    (["-k", "21", "-i", "a.fq", "--target", "8"], "the following arguments are required: -o/--output"),
    (_BASE + ["--target", "eight"], "argument --target: invalid int value: 'eight'"),
    (_BASE + ["--target", "8.5"], "argument --target: invalid int value: '8.5'"),
    (_BASE + ["--target", "8", "-U", "9"], "unrecognized arguments: -U 9"),
    (_BASE + ["--target", "8", "--min-hits", "3"], "unrecognized arguments: --min-hits 3"),
]


def _files(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for name in ("a.fq", "b.fq", "t.fq", "t.dump"):
        (tmp_path / name).write_bytes(b"")
    return ["a.fq", "b.fq", "t.dump", "t.fq"]


@pytest.mark.parametrize("argv,reason", _REFUSED, ids=[" ".join(a) for a, _ in _REFUSED])
def test_kmer_table_normalize_refuses_for_the_reason(argv, reason, capsys, tmp_path, monkeypatch):
    """the check that refuses the arguments is the one named: ``_normalize_plan`` raises it, before anything touches a device, and
    the tool ends with status 1 and that very message"""
    before = _files(tmp_path, monkeypatch)
    with pytest.raises(ValueError, match=reason):
        _plan(argv)
    assert _main(["normalize"] + argv) == 1
    out = capsys.readouterr()
    assert out.out == "" and re.fullmatch(r"kmer_table: .*" + reason + r".*\n", out.err), out.err
    assert sorted(os.listdir(tmp_path)) == before


@pytest.mark.parametrize("argv,words", _UNPARSED, ids=[" ".join(a) for a, _ in _UNPARSED])
def test_kmer_table_normalize_unparsed_arguments_exit_1(argv, words, capsys, tmp_path, monkeypatch):
    before = _files(tmp_path, monkeypatch)
    assert _main(["normalize"] + argv) == 1
    out = capsys.readouterr()
    assert out.out == "" and words in out.err and out.err.startswith("usage: kmer_table")
    assert sorted(os.listdir(tmp_path)) == before


# ------------------------------------------------------------------------------------------------------------ the reference

def test_the_draw_known_answers():
    assert ref.draw(0, 0) == 14819496
    assert ref.draw(0, 1) == 7239838
    assert ref.draw(2023, 12345) == 12206996
    assert ref.draw((1 << 64) - 1, (1 << 40) + 7) == 8941301
    assert all(0 <= ref.draw(s, u) < 1 << 24 for s in (0, 1, (1 << 64) - 1) for u in range(50))


def _code(s: str) -> int:
    """canonical code of a k-mer string, by string operations alone: A0 C1 T2 G3, first character highest, the smaller strand"""
    rc = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    return min(int("".join(str("ACTG".index(c)) for c in x), 4) for x in (s, rc))


def _items(table: dict):
    pairs = sorted((_code(s), c) for s, c in table.items())
    return np.array([p[0] for p in pairs], np.uint64), np.array([p[1] for p in pairs], np.int64)


# k = 3.  The made-up table holds the 3-mers of ACGACAAC (and their other strands): ACG (= CGT) 5, CGA (= TCG) 5, GAC (= GTC) 5,
# ACA (= TGT) 2, CAA (= TTG) 9, AAC (= GTT) 2
TABLE = {"ACG": 5, "CGA": 5, "GAC": 5, "AAC": 2, "ACA": 2, "CAA": 9}


def _rec(name: bytes, seq: bytes, qual: bytes = None, eol: bytes = b"\n", last: bytes = None) -> bytes:
    qual = b"I" * len(seq) if qual is None else qual
    return b"@" + name + eol + seq + eol + b"+" + eol + qual + (eol if last is None else last)


def test_reference_rows_written_out_by_hand():
    items, k = _items(TABLE), 3

    def one(seq, qual=None, **kw):
        return ref.read_depths(_rec(b"r", seq, qual), k, items, **kw)[0].tolist()

    # ACG CGA GAC ACA CAA AAC: 5 5 5 2 9 2, ascending 2 2 5 5 5 9; index (5 * p) // 100
    assert one(b"ACGACAAC") == [6, 6, 5]                                           # 250 // 100 = 2
    assert one(b"ACGACAAC", percentile=0) == [6, 6, 2]
    assert one(b"ACGACAAC", percentile=25) == [6, 6, 2]                            # 125 // 100 = 1
    assert one(b"ACGACAAC", percentile=54) == [6, 6, 5]                            # 270 // 100 = 2
    assert one(b"ACGACAAC", percentile=60) == [6, 6, 5]                            # 300 // 100 = 3
    assert one(b"ACGACAAC", percentile=99) == [6, 6, 5]                            # 495 // 100 = 4
    assert one(b"ACGACAAC", percentile=100) == [6, 6, 9]
    # lower = 3: the 2s count as 0: 0 0 5 5 5 9
    assert one(b"ACGACAAC", lower=3) == [6, 4, 5]
    assert one(b"ACGACAAC", lower=3, percentile=25) == [6, 4, 0]
    assert one(b"ACGACAAC", lower=6) == [6, 1, 0] and one(b"ACGACAAC", lower=6, percentile=100) == [6, 1, 9]
    assert one(b"ACGACAAC", lower=10, percentile=100) == [6, 0, 0]
    # CAA AAC ACA CAA: 9 2 2 9 -> 2 2 9 9; the LOWER median: index 150 // 100 = 1
    assert one(b"CAACAA") == [4, 4, 2] and one(b"CAACAA", percentile=67) == [4, 4, 9]
    # absent k-mers only: TTT (= AAA) is not in the table
    assert one(b"TTTTT") == [3, 0, 0] and one(b"TTTTT", percentile=100) == [3, 0, 0]
    # no k-mer at all
    assert one(b"AC") == [0, 0, 0] and one(b"") == [0, 0, 0] and one(b"ACNACNNA") == [0, 0, 0]
    # an N takes its three k-mers away: ACG | . . . | CAA AAC
    assert one(b"ACGNCAAC") == [3, 3, 5]
    # lower case: bases under lowercase_is_base; otherwise positions 2 .. 4 hold no k-mer: ACG CGA | AAC -> 2 5 5
    assert one(b"ACGAcAAC") == [6, 6, 5] and one(b"ACGAcAAC", lowercase_is_base=False) == [3, 3, 5]
    # the quality threshold masks base 0: CGA GAC ACA CAA AAC -> 2 2 5 5 9, index 2
    assert one(b"ACGACAAC", b"#IIIIIII", min_qual_char="?") == [5, 5, 5]
    # '\r' is a byte of its line and no base: the same six k-mers
    assert ref.read_depths(_rec(b"c", b"ACGACAAC", eol=b"\r\n"), k, items).tolist() == [[6, 6, 5]]
    with pytest.raises(ref.Malformed) as e:
        ref.read_depths(_rec(b"g", b"ACGAC") + _rec(b"short", b"ACGAC", b"IIII"), k, items, min_qual_char="?")
    assert e.value.record == 1
    assert ref.read_depths(b"", k, items).shape == (0, 3)


def test_reference_kept_records_written_out_by_hand():
    """four records: d = 5, 2, 0 (absent k-mers only), and one without k-mers.  The draws of units 0 and 1 under seed 0 are the
    known answers 14819496 and 7239838; target 4 is 4 * 2^24 = 67108864"""
    items, k = _items(TABLE), 3
    r0, r1, r2, r3 = _rec(b"a/1", b"ACGACAAC"), _rec(b"a/2", b"CAACAA"), _rec(b"b/1", b"TTTTT"), _rec(b"b/2", b"AC", last=b"")
    data = r0 + r1 + r2 + r3
    assert ref.read_depths(data, k, items).tolist() == [[6, 6, 5], [4, 4, 2], [3, 0, 0], [0, 0, 0]]
    assert 14819496 * 5 >= 67108864 > 14819496 * 2 and 7239838 * 2 < 67108864
    # interleaved: unit 0 = records 0, 1 (w = 14819496): 5 fails, 2 passes; unit 1 = records 2, 3 (w = 7239838): d = 0 passes the
    # draw always, the record without k-mers never passes
    totals = {"records": 4, "passed": 2, "low": 1, "bases": 21, "kmers": 13, "hits": 10, "depth_in": 7}
    o1, o2, tot = ref.normalize_fastq(data, k, items, target=4)
    assert o1 == data and o2 is None and tot == dict(totals, kept=4, depth_out=7)
    o1, o2, tot = ref.normalize_fastq(data, k, items, target=4, pair="both")
    assert o1 == b"" and tot == dict(totals, kept=0, depth_out=0)
    # min_depth 1: the absent-only read is low too, its pair goes
    o1, _, tot = ref.normalize_fastq(data, k, items, target=4, min_depth=1)
    assert o1 == r0 + r1 and tot == dict(totals, passed=1, low=2, kept=2, depth_out=7)
    # target 5: 5 * 2^24 = 83886080 > 14819496 * 5 = 74097480: record 0 passes too
    o1, _, tot = ref.normalize_fastq(data, k, items, target=5, pair="both")
    assert o1 == r0 + r1 and tot == dict(totals, passed=3, kept=2, depth_out=7)
    # R1 / R2: record i of both files is unit i -- the same mates, the same draws
    o1, o2, tot = ref.normalize_fastq(r0 + r2, k, items, r1 + r3, target=4)
    assert o1 == r0 + r2 and o2 == r1 + r3 and tot == dict(totals, kept=4, depth_out=7)
    o1, o2, tot = ref.normalize_fastq(r0 + r2, k, items, r1 + r3, target=4, min_depth=1, pair="any")
    assert o1 == r0 and o2 == r1 and tot == dict(totals, passed=1, low=2, kept=2, depth_out=7)
    # single: every record is its own unit: record 0 draws 14819496 (fails at d = 5), record 1 draws 7239838 (passes at d = 2)
    o1, _, tot = ref.normalize_fastq(r0 + r1, k, items, target=4, pair="single")
    assert o1 == r1 and tot == {"records": 2, "kept": 1, "passed": 1, "low": 0, "bases": 14, "kmers": 10, "hits": 10, "depth_in": 7, "depth_out": 2}
    # the percentile reaches the rule: at the maximum record 1 has d = 9: 14819496 * 9 > 67108864, nobody of unit 0 passes
    o1, _, tot = ref.normalize_fastq(data, k, items, target=4, percentile=100)
    assert o1 == r2 + r3 and tot["passed"] == 1 and tot["depth_in"] == 18 and tot["depth_out"] == 0
    # another seed, other draws
    assert ref.draw(1, 0) != ref.draw(0, 0)
    with pytest.raises(ref.Malformed):
        ref.normalize_fastq(r0 + r1 + r2, k, items, target=4)                     # an odd number of records under any
    with pytest.raises(ref.Malformed):
        ref.normalize_fastq(r0 + r2, k, items, r1, target=4)
