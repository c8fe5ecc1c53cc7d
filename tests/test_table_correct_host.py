"""The read-correcting entry (pg_table_correct_reads: single substitutions in the reads of a FASTQ text put right from a k-mer
table, beside scripts/low_abd_reads.sh:10 / extract_unmapped.cpp) as far as the host decides about it: declared, exported,
mirrored in ``_lib``, every refusal returned BEFORE the first HIP call -- descriptors and buffers carry fake addresses that are
never dereferenced --, the argument handling of ``kmer_table correct``, and the reference the GPU tests compare with
(tests/_correct_ref.py) on examples whose answers are written out by hand, with its two theorems on random reads.  No kernel is
launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pangaea_amd import _lib, cli

from . import _correct_ref as ref
from . import _filter_ref
from .conftest import ROOT

OK, EINVAL = 0, -1
FAKE = 0x7F0000000000            # a 256-byte aligned address that belongs to nobody
WHO = "pg_table_correct_reads"


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
    assert re.search(r"int\s+pg_table_correct_reads\s*\(\s*const pg_table \*t,\s*int k,\s*const uint8_t \*text,\s*int64_t n_bytes,\s*"
                     r"const int64_t \*line_start,\s*int64_t n_records,\s*int64_t first_record,\s*int64_t lower,\s*int64_t upper\s*,\s*"
                     r"int lowercase_is_base,\s*int min_qual_char\s*,\s*uint8_t \*out\s*,\s*uint32_t \*rows\s*,\s*"
                     r"uint64_t \*status\s*,\s*void \*stream\s*\)", code)
    assert re.search(WHO + r"\s+beside scripts/low_abd_reads\.sh:10 / extract_unmapped\.cpp", hdr)
    assert "Single substitutions in the reads of a FASTQ text put right" in hdr
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, WHO) and WHO in _lib.EXPORTS
    assert _lib.load().pg_table_correct_reads.argtypes is not None and len(_lib.load().pg_table_correct_reads.argtypes) == 15


# (t, k, text, n_bytes, line_start, n_records, first_record, lower, upper, lowercase_is_base, min_qual_char, out, rows, status)
_GOOD = (_table(), 21, FAKE, 1000, FAKE, 4, 0, 1, -1, 1, 0, FAKE, FAKE, FAKE)
_NAMES = ("t", "k", "text", "n_bytes", "line_start", "n_records", "first_record", "lower", "upper", "lowercase_is_base", "min_qual_char", "out",
          "rows", "status")


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
    (_with(lower=-1), WHO + ": lower is negative (-1)"),
    (_with(lower=6, upper=5), WHO + ": upper 5 is below lower 6"),
    (_with(lower=1, upper=0), WHO + ": upper 0 is below lower 1"),
    (_with(min_qual_char=256), WHO + ": min_qual_char 256 is no byte (0: none)"),
    (_with(min_qual_char=-1), WHO + ": min_qual_char -1 is no byte (0: none)"),
    (_with(text=FAKE + 4), WHO + ": text is not 16-byte aligned"),
    (_with(text=FAKE + 4, out=None), WHO + ": text is not 16-byte aligned"),
    (_with(k=20), WHO + ": k differs (table 21, asked 20)"),
    (_with(t=_table(kind=9)), "unknown table kind 9"),
    (_with(t=_table(k=12), k=12), "mini table needs 13 <= k <= 21 (got 12)"),
    (_with(t=_table(kind=_lib.TABLE_DENSE, k=17), k=17), "dense table needs 1 <= k <= 16 (got 17)"),
    (_with(t=_table(data=None)), "table descriptor is null"),
])
def test_correct_reads_refusals(args, text):
    t = args[0]
    rc, msg = _call(WHO, None if t is None else C.byref(t), *args[1:], None)
    assert rc == EINVAL and msg == text


def test_nothing_asked_is_ok_and_launches_nothing():
    for t in (_table(), _table(kind=_lib.TABLE_WIDE, k=31, log2_bucket_slots=0), _table(kind=_lib.TABLE_DENSE, k=4)):
        for out in (None, FAKE + 16, FAKE):                      # rows only, an out buffer, in place
            assert _call(WHO, C.byref(t), t.k, FAKE, 0, FAKE, 0, 0, 0, 0, 1, 0, out, FAKE, FAKE, None)[0] == OK


# ------------------------------------------------------------------------------------------------------------ the tool

def _main(argv):
    try:
        return cli.main_kmer_table(argv)
    except SystemExit as e:
        return e.code


def _plan(argv):
    return cli._correct_plan(cli._kmer_table_parser().parse_args(["correct"] + argv))


def test_kmer_table_correct_arguments_accepted(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for name in ("a.fq", "b.fq", "t.fq", "u.fq", "t.dump"):
        (tmp_path / name).write_bytes(b"")
    src, reads, kw = _plan(["-k", "21", "-i", "a.fq", "-o", "out.fq"])
    assert src is None and reads == ("a.fq", None, "out.fq", None)
    assert kw == dict(lower=1, upper=None, min_qual_char=None, lowercase_is_base=True)
    src, reads, kw = _plan(["-g", "t.dump", "-k", "15", "-1", "a.fq", "-2", "b.fq", "-o", "o1.fq", "-o2", "o2.fq", "-L", "2", "-U", "9",
                            "--min-qual-char", "?"])
    assert src == ("dump", "t.dump") and reads == ("a.fq", "b.fq", "o1.fq", "o2.fq")
    assert kw == dict(lower=2, upper=9, min_qual_char="?", lowercase_is_base=True)
    src, _, _ = _plan(["-ti", "t.fq", "-k", "31", "-i", "a.fq", "-o", "out.fq"])
    assert src == ("reads", "t.fq", None)
    src, _, _ = _plan(["-t1", "t.fq", "-t2", "u.fq", "-k", "21", "-i", "a.fq", "-o", "out.fq"])
    assert src == ("reads", "t.fq", "u.fq")
    monkeypatch.setenv("PANGAEA_LOWERCASE_IS_BASE", "0")
    assert _plan(["-k", "21", "-i", "a.fq", "-o", "out.fq"])[2]["lowercase_is_base"] is False
    assert sorted(os.listdir(tmp_path)) == ["a.fq", "b.fq", "t.dump", "t.fq", "u.fq"]


def test_kmer_table_correct_help_says_what_lower_makes_sense(capsys):
    assert _main(["correct", "--help"]) == 0
    out = capsys.readouterr().out
    assert "-L 2 or more" in " ".join(out.split())


# (arguments, the reason ``_correct_plan`` gives -- a regular expression): what ``_trim_plan`` refuses for the shared options
_REFUSED = [
    (["-k", "21", "-o", "out.fq"], r"the reads to correct are -i F or -1 F -2 F"),                                     # no reads
    (["-k", "40", "-i", "a.fq", "-o", "out.fq"], r"k-mer size 40 unsupported"),
    (["-k", "0", "-i", "a.fq", "-o", "out.fq"], r"k-mer size 0 unsupported"),
    (["-k", "21", "-i", "a.fq", "-1", "a.fq", "-2", "b.fq", "-o", "out.fq", "-o2", "o2.fq"], r"-i F or -1 F -2 F \(one of the two\)"),
    (["-k", "21", "-1", "a.fq", "-o", "out.fq"], r"-1 and -2 go together"),
    (["-k", "21", "-2", "b.fq", "-o", "out.fq"], r"-1 and -2 go together"),
    (["-k", "21", "-1", "a.fq", "-2", "b.fq", "-o", "out.fq"], r"writes two files: -o OUT -o2 OUT2"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "-o2", "o2.fq"], r"-o2 goes with -1 F -2 F"),
    (["-k", "21", "-g", "t.dump", "-ti", "t.fq", "-i", "a.fq", "-o", "out.fq"], r"correct takes the table from one source"),
    (["-k", "21", "-g", "t.dump", "-t1", "t.fq", "-t2", "t.fq", "-i", "a.fq", "-o", "out.fq"], r"correct takes the table from one source"),
    (["-k", "21", "-t1", "t.fq", "-i", "a.fq", "-o", "out.fq"], r"-t1 and -t2 go together"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "-L=-2"], r"-L must be at least 0 \(got -2\)"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "-L", "5", "-U", "4"], r"-U \(4\) is below -L \(5\)"),
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
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "-L", "two"], "argument -L/--lower-count: invalid int value: 'two'"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--pair", "any"], "unrecognized arguments: --pair any"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--min-len", "3"], "unrecognized arguments: --min-len 3"),
    (["-k", "21", "-i", "a.fq", "-o", "out.fq", "--min-hits", "3"], "unrecognized arguments: --min-hits 3"),
]


def _files(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for name in ("a.fq", "b.fq", "t.fq", "t.dump"):
        (tmp_path / name).write_bytes(b"")
    return ["a.fq", "b.fq", "t.dump", "t.fq"]


@pytest.mark.parametrize("argv,reason", _REFUSED, ids=[" ".join(a) for a, _ in _REFUSED])
def test_kmer_table_correct_refuses_for_the_reason(argv, reason, capsys, tmp_path, monkeypatch):
    """the check that refuses the arguments is the one named: ``_correct_plan`` raises it, before anything touches a device, and
    the tool ends with status 1 and that very message"""
    before = _files(tmp_path, monkeypatch)
    with pytest.raises(ValueError, match=reason):
        _plan(argv)
    assert _main(["correct"] + argv) == 1
    out = capsys.readouterr()
    assert out.out == "" and re.fullmatch(r"kmer_table: .*" + reason + r".*\n", out.err), out.err
    assert sorted(os.listdir(tmp_path)) == before


@pytest.mark.parametrize("argv,words", _UNPARSED, ids=[" ".join(a) for a, _ in _UNPARSED])
def test_kmer_table_correct_unparsed_arguments_exit_1(argv, words, capsys, tmp_path, monkeypatch):
    before = _files(tmp_path, monkeypatch)
    assert _main(["correct"] + argv) == 1
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


# k = 3.  The made-up table holds the 3-mers of ACGACAAC (and their other strands): ACG (= CGT) 5, CGA (= TCG) 5, GAC (= GTC) 5,
# ACA (= TGT) 2, CAA (= TTG) 9, AAC (= GTT) 2
TABLE = {"ACG": 5, "CGA": 5, "GAC": 5, "AAC": 2, "ACA": 2, "CAA": 9}


def _rec(name: bytes, seq: bytes, qual: bytes = None, eol: bytes = b"\n", last: bytes = None) -> bytes:
    qual = b"I" * len(seq) if qual is None else qual
    return b"@" + name + eol + seq + eol + b"+" + eol + qual + (eol if last is None else last)


def test_candidates_of_class_strings():
    c = ref.candidates_of
    assert c("", 3) == [] and c("SSSS", 3) == [] and c("WWW", 3) == [] and c("W", 3) == []                 # E on both sides
    assert c("SSWWWS", 3) == [(2, 5, 4)] and c("SSWWS", 3) == [] and c("SWWWWS", 3) == [] and c("SWS", 3) == []
    assert c("WWSS", 3) == [(0, 2, 1)] and c("WSS", 3) == [(0, 1, 0)] and c("WWWS", 3) == [(0, 3, 2)] and c("WWWWS", 3) == []
    assert c("SSWW", 3) == [(2, 4, 4)] and c("SW", 3) == [(1, 2, 3)] and c("SWWW", 3) == [(1, 4, 3)] and c("SWWWW", 3) == []
    assert c("VWWWS", 3) == [] and c("SWWWV", 3) == [] and c("VWW", 3) == [] and c("WWV", 3) == []          # a V neighbour
    assert c("WSWWWSW", 3) == [(0, 1, 0), (2, 5, 4), (6, 7, 8)]
    assert c("SWWWSWWWS", 3) == [(1, 4, 3), (5, 8, 7)]


def test_reference_on_records_written_out_by_hand():
    items = _items(TABLE)
    k = 3

    def one(seq, qual=None, **kw):
        rows, out, gained, _ = ref.read_corrections(_rec(b"r", seq, qual), k, items, **kw)
        assert out[:3] == b"@r\n" and out[3 + len(seq):] == b"\n+\n" + (qual or b"I" * len(seq)) + b"\n"
        return rows[0].tolist(), out[3:3 + len(seq)], int(gained[0])

    # no error: ACG CGA GAC ACA CAA AAC, all solid
    assert one(b"ACGACAAC") == ([6, 6, 0, 0], b"ACGACAAC", 0)
    # S .. S, b - a == k: ACG CGA | GAG AGA GAA | AAC: run [2, 5), p = 4.  A there: GAA AAA AAC -- no; C: GAC ACA CAA -- all
    # three; T: GAT ATA TAA -- no
    assert one(b"ACGAGAAC") == ([6, 3, 1, 1], b"ACGACAAC", 3)
    # E .. S: AGG GGA | GAC ACA CAA AAC: run [0, 2), p = 1.  C: ACG CGA -- both; A: AAG -- no; T: ATG -- no
    assert one(b"AGGACAAC") == ([6, 4, 1, 1], b"ACGACAAC", 2)
    # S .. E: ACG CGA GAC ACA | CAT ATC: run [4, 6), p = 4 + k - 1 = 6.  A: CAA AAC; C: CAC -- no; G: CAG -- no
    assert one(b"ACGACATC") == ([6, 4, 1, 1], b"ACGACAAC", 2)
    # S .. E with one weak k-mer: the last base.  AAG: p = 5 + 2 = 7; C gives AAC, A gives AAA, T gives AAT
    assert one(b"ACGACAAG") == ([6, 5, 1, 1], b"ACGACAAC", 1)
    # an interior run of k - 1 (AAC ACA | CAG AGA | GAC) and one of k + 1 (AAC | ACC CCA CAG AGA | GAC): no candidates
    assert one(b"AACAGAC") == ([5, 3, 0, 0], b"AACAGAC", 0)
    assert one(b"AACCAGAC") == ([6, 2, 0, 0], b"AACCAGAC", 0)
    # a V neighbour: the quality threshold masks base 6, so positions 4 and 5 hold no k-mer and the run [2, 4) ends at a void one
    assert one(b"ACGAGAAC", b"IIIIII#I", min_qual_char="?") == ([4, 2, 0, 0], b"ACGAGAAC", 0)
    # ... while a masked base in front leaves the run between two solid positions: V S W W W S
    assert one(b"ACGAGAAC", b"#IIIIIII", min_qual_char="?") == ([5, 2, 1, 1], b"ACGACAAC", 3)
    # an N beside the error: ACG | CGN GNG NGA (void) | GAA (weak) | AAC: the run's left neighbour is void
    assert one(b"ACGNGAAC") == ([3, 2, 0, 0], b"ACGNGAAC", 0)
    # E on both sides: TTT (= AAA) is not in the table, the read is weak throughout
    assert one(b"TTTTT") == ([3, 0, 0, 0], b"TTTTT", 0)
    # ambiguous: ACG CGA GAC | ACT CTA TAC, p = 5.  A: ACA CAA AAC; G: ACG CGA GAC -- two valid bases, the byte stays
    assert one(b"ACGACTAC") == ([6, 3, 1, 0], b"ACGACTAC", 0)
    # no valid base: AAC | ACC CCC CCA | CAA, p = 3: A: ACA CAC -- no; G: ACG CGC -- no; T: ACT -- no
    assert one(b"AACCCAA") == ([5, 2, 1, 0], b"AACCCAA", 0)
    assert one(b"AACAAAT") == ([5, 3, 1, 0], b"AACAAAT", 0)     # ... and at the end: AAC ACA CAA | AAA AAT, p = 5
    # lower case: a base under lowercase_is_base, corrected in lower case; no base otherwise (positions 2 .. 4 void)
    assert one(b"ACGAgAAC") == ([6, 3, 1, 1], b"ACGAcAAC", 3)
    assert one(b"ACGAgAAC", lowercase_is_base=False) == ([3, 3, 0, 0], b"ACGAgAAC", 0)
    assert one(b"ACGAcAAC") == ([6, 6, 0, 0], b"ACGAcAAC", 0)
    # two candidates of one record, both corrected: AAA AAA | AAC ACA | CAC: [0, 2) with p = 1 and [4, 5) with p = 6
    assert one(b"AAAACAC") == ([5, 2, 2, 2], b"ACAACAA", 3)
    # the window: under [2, 5] CAA (9) is weak: ACG CGA GAC ACA | CAA | AAC is an interior run of 1
    assert one(b"ACGACAAC", lower=2, upper=5) == ([6, 5, 0, 0], b"ACGACAAC", 0)
    assert one(b"ACGACAAC", lower=0, upper=0) == ([6, 0, 0, 0], b"ACGACAAC", 0)
    # CRLF with a right-end error: the '\r' is beyond the end, so the run [4, 6) reaches E and is corrected; the '\r' stays
    crlf = _rec(b"c", b"ACGACATC", eol=b"\r\n")
    rows, out, gained, det = ref.read_corrections(crlf, k, items)
    assert rows.tolist() == [[6, 4, 1, 1]] and out == _rec(b"c", b"ACGACAAC", eol=b"\r\n") and det[0] == [(4, 6, 6, [ord("A")])]
    assert rows[:, :2].tolist() == _filter_ref.read_hits(crlf, k, items).tolist()
    # no final newline; records do not interact
    two = _rec(b"a", b"AGGACAAC") + _rec(b"b", b"ACGACAAG", b"ABCDEFGH", last=b"")
    rows, out, gained, _ = ref.read_corrections(two, k, items)
    assert rows.tolist() == [[6, 4, 1, 1], [6, 5, 1, 1]] and gained.tolist() == [2, 1]
    assert out == b"@a\nACGACAAC\n+\nIIIIIIII\n@b\nACGACAAC\n+\nABCDEFGH"
    o1, o2, tot = ref.correct_fastq(two, k, items)
    assert o1 == out and o2 is None
    assert tot == {"records": 2, "bases": 16, "kmers": 12, "hits": 9, "candidates": 2, "corrected": 2, "reads_corrected": 2}
    o1, o2, tot = ref.correct_fastq(_rec(b"p1", b"ACGACTAC"), k, items, _rec(b"p2", b"AAAACAC"))
    assert o1 == _rec(b"p1", b"ACGACTAC") and o2 == _rec(b"p2", b"ACAACAA")
    assert tot == {"records": 2, "bases": 15, "kmers": 11, "hits": 5, "candidates": 3, "corrected": 2, "reads_corrected": 1}
    with pytest.raises(ref.Malformed):
        ref.correct_fastq(two, k, items, _rec(b"p2", b"AAAACAC"))
    with pytest.raises(ref.Malformed) as e:
        ref.read_corrections(_rec(b"g", b"ACGAC") + _rec(b"short", b"ACGAC", b"IIII"), k, items)
    assert e.value.record == 1
    assert ref.read_corrections(b"", k, items)[1] == b""


@pytest.mark.parametrize("k", [5, 9])
def test_the_two_theorems_on_random_reads(k):
    """after the pass h has grown by exactly the corrected runs' lengths, and a second pass finds candidates - corrected candidates
    and corrects none -- on 300 reads with zero to three planted substitutions, N's among them"""
    rng = np.random.default_rng(100 + k)
    genome = "".join(rng.choice(list("ACGT"), 600 if k == 9 else 150))
    table = {}
    for i in range(len(genome) - k + 1):
        table[genome[i:i + k]] = table.get(genome[i:i + k], 0) + 1
    merged = {}
    for s, c in table.items():
        merged[_code(s)] = merged.get(_code(s), 0) + c
    codes = np.array(sorted(merged), np.uint64)
    items = (codes, np.array([merged[int(c)] for c in codes], np.int64))
    recs = []
    for r in range(300):
        n = int(rng.integers(k, 120))
        at = int(rng.integers(0, len(genome) - n + 1))
        seq = bytearray(genome[at:at + n].encode())
        for _ in range(int(rng.integers(0, 4))):
            p = int(rng.integers(0, n))
            seq[p] = rng.choice([c for c in b"ACGTN" if c != seq[p]])
        if r % 7 == 0:
            seq = bytearray(bytes(seq).lower()[:n // 2] + bytes(seq)[n // 2:])
        recs.append(_rec(b"r%d" % r, bytes(seq)))
    data = b"".join(recs)
    for window in ((1, None), (1, 1)):
        rows, out, gained, _ = ref.read_corrections(data, k, items, *window)
        assert rows[:, :2].tolist() == _filter_ref.read_hits(data, k, items, *window).tolist()
        # (the theorems say something only if some candidates are corrected and some are left: neither all nor nothing)
        assert rows[:, 3].sum() >= 1 and (rows[:, 2] > rows[:, 3]).sum() >= 1, rows.sum(0)
        again, out2, gained2, _ = ref.read_corrections(out, k, items, *window)
        assert out2 == out and not gained2.any()
        assert again[:, 0].tolist() == rows[:, 0].tolist()
        assert again[:, 1].tolist() == (rows[:, 1] + gained).tolist()
        assert again[:, 2].tolist() == (rows[:, 2] - rows[:, 3]).tolist() and not again[:, 3].any()
        assert _filter_ref.read_hits(out, k, items, *window)[:, 1].tolist() == (rows[:, 1] + gained).tolist()
