"""Reads of a FASTQ file cut down to their solid k-mer span: ``KmerTable.read_spans`` / ``KmerTable.trim_fastq`` (pg_fastq_index,
pg_table_read_spans, pg_fastq_gather_trimmed) and ``kmer_table trim`` -- what `kmc_tools filter -t` and khmer's filter-abund do,
beside the read set of scripts/low_abd_reads.sh:10 (extract_unmapped.cpp).

Everything is integers and bytes, compared exactly with tests/_trim_ref.py (a numpy restatement of the semantics in
include/pangaea_feat.h).  The tables are the six of tests/test_table_filter_gpu.py (built once per session, shared with those
tests, compared with their clones after every test); the corpus is that module's ``corpus_of`` plus the RUN-STRUCTURE records of
``structures``: stretches S(p) of p + k - 1 characters that give p solid positions, joined with one N (k positions without a
k-mer), placed so that runs end, begin, tie and carry on at the 64-position ballot words and the 512-position batches of the
kernel.  Every structure is built from three materials, because no single one is solid for every table:
  own      p + k - 1 consecutive characters of the table's own text without its separators: solid under [1, none] -- exactly so
           for the dense k = 4 table, which holds every 4-mer; for k >= 13 the k-mers across two reads of the text are not in the
           table, so these are runs of at most 150 - k + 1 positions with gaps where the reads meet;
  foreign  random characters: solid under the window (0, 0), the absent k-mers -- exactly so for k >= 21; a random 13-mer is in
           the k = 13 table once in a few hundred positions;
  poly     A A A ... : one k-mer, absent from every table of k >= 13 and present in the dense one, so that these records have
           EXACTLY the designed runs under one of the windows of every table -- ``test_the_designed_runs_are_there`` asserts that
           on the reference, run by run, and so what the kernel is compared with does contain a run across more than two
           batches, a tie across a word boundary and the rest.

THE BAND.  Every ``trim_fastq`` case is asserted, on the reference's own result, to keep between 10 % and 90 % of the records and
to shorten between 10 % and 90 % of the kept ones, so that no case passes by keeping all or nothing or by copying whole
records.  Cases: both modes, ``min_len`` in {k, 50}, the five (form, pair) combinations of the filter tests, the window [1, none].
Left out, because the reference itself is outside the band there (``combos_of``):
  * mini k = 13 / longest / any / min_len = 13: a random 13-mer is in the table by chance often enough that almost every read
    has a solid position; that combination keeps 89.9 % of the filter corpus, too close to the edge;
  * the dense k = 4 table.  Every 4-mer is in it, so its window is the filter tests' ``window_of`` (the count that half of the
    table's occurrences reach): hits are coin flips, ``longest`` keeps 98 % and more, any ``min_len`` >= 8 under 13 % under
    ``first``, and 99 % of the kept reads are shortened.  Only ``first`` with ``min_len = 4`` is run there, and only the first
    band (the records kept) is asserted.
``test_long_spans_leave_whole`` adds the window (0, 0) on the k >= 21 tables, where the foreign and poly structures are solid
from end to end: spans of thousands of bases through the gather, inside the same band.  The window (2, none) keeps under 10 % on
the 40-pair mini k = 21 table and is used for ``read_spans`` only."""
import gzip
import json
import os

import numpy as np
import pytest
import torch

from pangaea_amd import cli, synth

from . import _trim_ref as ref
from .test_table_filter_gpu import CASES, DEV, FORMS, _IDS, _built, _record, _synth_cfg, window_of

pytestmark = pytest.mark.gpu

WINDOWS = [(1, None), (2, 5), (0, 0), (2, None)]
MODES = ("first", "longest")


def structures(S, k: int, tag: bytes) -> list:
    """the run-structure records of one material: ``S(p)`` gives p + k - 1 characters meant as p solid positions.  (name, sequence,
    the designed runs [(a, b)] when every S(p) is solid from end to end and nothing else is)"""
    out = []

    def add(name, *parts):
        seq, runs, at = b"", [], 0
        for p in parts:
            if p == "N":
                seq += b"N"
                at += 1
            else:
                seq += S(p)
                if p:
                    runs.append((at, at + p))
                at += p + k - 1
        out.append((tag + b" " + name, seq, runs))

    add(b"S64", 64)                                  # within and across one ballot word
    add(b"S63 N S65", 63, "N", 65)
    add(b"S64 N S64", 64, "N", 64)                   # a tie: the first wins
    add(b"S65 N S63", 65, "N", 63)
    add(b"S300 N S700", 300, "N", 700)               # across the 512-position batch: the longest is the second, FIRST the first
    add(b"N S1500 N S100", "N", 1500, "N", 100)      # a run over more than two batches
    add(b"S200 N S400 N S200", 200, "N", 400, "N", 200)      # the last run (a tie for second place) lies beyond position 512
    add(b"S1 N S1 N S2 N S1", 1, "N", 1, "N", 2, "N", 1)     # single-position runs: the 2-position run wins
    add(b"S1", 1)                                    # length exactly k
    add(b"S30 N S70", 30, "N", 70)                   # a run that ends at the read's last position
    add(b"S70 N", 70, "N")                           # a read that ends in N
    add(b"N S70", "N", 70)                           # a read that begins with N: FIRST gives an empty span, LONGEST does not
    add(b"S100", 100)                                # all solid
    add(b"S0", 0)                                    # length k - 1
    add(b"S512 N S512", 512, "N", 512)               # a tie of two whole batches
    add(b"S5000", 5000)                              # a long read
    return out


def trim_corpus(text: bytes, records: list, k: int, seed: int) -> tuple:
    """(the filter tests' records plus the run-structure records -- an even number, mates next to each other --, {name: designed
    runs} of the poly material)"""
    rng = np.random.RandomState(seed)
    clean = np.frombuffer(text.replace(b"N", b""), np.uint8)
    at = [len(clean) // 3]

    def own(p):                                      # consecutive characters of the table's text, going round at its end
        n = p + k - 1
        idx = (at[0] + np.arange(n)) % len(clean)
        at[0] += n
        return bytes(clean[idx])

    def foreign(p):
        return bytes(rng.choice(list(b"ACGT"), p + k - 1).astype(np.uint8))

    def poly(p):
        return b"A" * (p + k - 1)

    recs, designed = list(records), {}
    for S, tag in ((own, b"own"), (foreign, b"foreign"), (poly, b"poly")):
        for name, seq, runs in structures(S, k, tag):
            recs.append(_record(name, seq))
            if tag == b"poly":
                designed[name] = runs
    recs.append(_record(b"empty sequence line", b""))
    recs.append(_record(b"k foreign characters", foreign(1)))
    recs.append(_record(b"own, lower case", own(100).lower()))
    recs.append(_record(b"own, low qualities", own(100), b"I" * 40 + b"#" + b"I" * 40 + b"4" + b"I" * (100 + k - 1 - 82)))
    if len(recs) % 2:
        recs.append(_record(b"the last one's mate", own(60)))
    return recs, designed


def combos_of(kind: str, k: int) -> list:
    """the (mode, min_len, form, pair) cases of a table's ``trim_fastq`` test (the module's docstring says which are left out)"""
    if k == 4:
        return [("first", 4, form, pair) for form, pair in FORMS]
    return [(mode, min_len, form, pair) for mode in MODES for min_len in (k, 50) for form, pair in FORMS
            if not (k == 13 and mode == "longest" and pair == "any" and min_len == 13)]


class _Corpus:
    def __init__(self, case):
        kind, k, log2_slots, _ = case
        self.b = b = _built(case)                    # the filter tests' table, items and corpus
        self.k, self.kind, self.table, self.items = k, kind, b.table, b.items
        cfg = _synth_cfg(k, log2_slots)
        text = synth.generate(cfg, device=DEV).decode()
        self.records, self.designed = trim_corpus(text, b.records, k, 900 + k)
        self.data = b"".join(self.records)
        self.r1, self.r2 = b"".join(self.records[0::2]), b"".join(self.records[1::2])
        self.window = window_of(k, self.items)
        self.cache = {}

    def unchanged(self):
        return self.b.unchanged()

    def want(self, form, pair, mode, min_len, window=None, **kw):
        lower, upper = window or self.window
        a, b = (self.data, None) if form == "interleaved" else (self.r1, self.r2)
        return ref.trim_fastq(a, self.k, self.items, b, lower=lower, upper=upper, mode=mode, min_len=min_len, pair=pair, cache=self.cache, **kw)


_CORPORA = {}


def _corpus(case):
    if case not in _CORPORA:
        _CORPORA[case] = _Corpus(case)
    return _CORPORA[case]


def _run(c, tmp_path, form, pair, mode, min_len, tag="x", data=None, window=None, **kw):
    """(bytes written 1, bytes written 2 or None, the returned dict) of ``trim_fastq`` on files written for the call"""
    lower, upper = window or c.window
    if form == "interleaved":
        src = tmp_path / f"{tag}.fq"
        src.write_bytes(c.data if data is None else data)
        out = tmp_path / f"{tag}.out.fq"
        res = c.table.trim_fastq(str(src), str(out), lower=lower, upper=upper, mode=mode, min_len=min_len, pair=pair, **kw)
        return out.read_bytes(), None, res
    s1, s2, o1, o2 = (tmp_path / f"{tag}.{n}.fq" for n in ("r1", "r2", "o1", "o2"))
    s1.write_bytes(c.r1 if data is None else data[0])
    s2.write_bytes(c.r2 if data is None else data[1])
    res = c.table.trim_fastq(str(s1), str(o1), str(s2), str(o2), lower=lower, upper=upper, mode=mode, min_len=min_len, pair=pair, **kw)
    return o1.read_bytes(), o2.read_bytes(), res


def _same(got, want):
    g1, g2, res = got
    w1, w2, tot = want
    assert g1 == w1 and g2 == w2
    assert {n: res[n] for n in tot} == tot
    assert set(res) == set(tot) | {"seconds", "device_ms"} and res["seconds"] > 0 and res["device_ms"] >= 0
    for n in tot:
        assert type(res[n]) is int


def _in_band(tot, what, second=True):
    kept, short = tot["kept"] / tot["records"], tot["trimmed"] / max(1, tot["kept"])
    print(f"{what}: the reference keeps {kept:.3f} and shortens {short:.3f} of those")
    assert 0.1 <= kept <= 0.9, (what, kept)
    if second:
        assert 0.1 <= short <= 0.9, (what, short)


# ------------------------------------------------------------------------------------------------------------ 1. read_spans

@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_the_designed_runs_are_there(case):
    """the reference, on the poly records, under the window that makes their one k-mer solid: exactly the designed runs"""
    c = _corpus(case)
    k = c.k
    per = ref.profiles_of(c.data, k, c.items, cache=c.cache)
    names = [r[1:r.index(b"\n")] for r in c.records]
    count = int(per[names.index(b"poly S1")][1][0])
    assert (count > 0) == (k == 4)                   # (poly-A: in the dense table, in no other)
    window = (1, None) if count else (0, 0)
    rows = {}
    for mode in MODES:
        rows[mode] = ref.read_spans(c.data, k, c.items, *window, mode=mode, cache=c.cache)
    assert len(c.designed) == 16
    for name, runs in c.designed.items():
        r = names.index(name)
        assert ref.runs_of(ref.solid_of(per[r], *window)) == runs, name
        longest = max(runs, key=lambda ab: ab[1] - ab[0], default=None)
        n = sum(b - a for a, b in runs)
        assert rows["longest"][r].tolist() == [n, n] + ([longest[0], longest[1] - longest[0] + k - 1] if runs else [0, 0]), name
        first = runs[0] if runs and runs[0][0] == 0 else None
        assert rows["first"][r].tolist() == [n, n] + ([0, first[1] + k - 1] if first else [0, 0]), name
    d = c.designed
    assert d[b"poly S64 N S64"] == [(0, 64), (64 + k, 128 + k)] and d[b"poly N S1500 N S100"][0] == (1, 1501)
    assert d[b"poly S200 N S400 N S200"][2][0] >= 512 and d[b"poly S300 N S700"][1] == (300 + k, 1000 + k)


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_read_spans_of_every_record(case):
    c = _corpus(case)
    text = torch.frombuffer(bytearray(c.data), dtype=torch.uint8).to(DEV)
    n_records = len(c.records)
    assert 400 <= n_records <= 440
    seen = set()
    asked = [(True, None, w, m) for w in WINDOWS for m in MODES]
    asked += [(lenient, mq, (1, None), m) for lenient, mq in ((False, None), (True, "5"), (False, "5")) for m in MODES]
    for lenient, mq, (lower, upper), mode in asked:
        got = c.table.read_spans(text, lower=lower, upper=upper, mode=mode, lowercase_is_base=lenient, min_qual_char=mq)
        assert got.dtype == torch.int64 and got.device == text.device and got.shape == (n_records, 4)
        want = ref.read_spans(c.data, c.k, c.items, lower, upper, mode, lenient, mq, cache=c.cache)
        bad = np.nonzero((got.cpu().numpy() != want).any(1))[0]
        assert len(bad) == 0, (lenient, mq, lower, upper, mode, bad[:5], got[bad[:5]], want[bad[:5]])
        seen.add(want.tobytes())
    assert len(seen) >= (10 if c.k > 4 else 6)       # (the windows, modes and rules ask different questions of this corpus)
    # n and h are those of read_hits, whatever the mode; a view that does not begin at a 16-byte boundary; nothing at all
    hits = c.table.read_hits(text)
    for mode in MODES:
        assert torch.equal(c.table.read_spans(text, mode=mode)[:, :2], hits)
    off = torch.cat([torch.zeros(3, dtype=torch.uint8, device=DEV), text])[3:]
    assert torch.equal(c.table.read_spans(off), c.table.read_spans(text))
    assert c.table.read_spans(text[:0]).shape == (0, 4)
    assert c.unchanged()


def test_read_spans_refuses_a_cpu_tensor_and_malformed_text():
    c = _corpus(CASES[1])
    good = c.records[0] + c.records[1]
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        c.table.read_spans(torch.frombuffer(bytearray(good), dtype=torch.uint8))

    def dev(data):
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)

    assert c.table.read_spans(dev(good)).shape == (2, 4)
    for data, record in ((good[:-5].rsplit(b"\n", 1)[0], 1), (good + b"\n", 2), (b"\n", 0), (good.replace(b"@", b"", 1), 0),
                         (c.records[0] + c.records[1].replace(b"\n+", b"\n-", 1) + c.records[2], 1)):
        with pytest.raises(ValueError, match=f"record {record}:"):
            c.table.read_spans(dev(data))
    # a short quality line is malformed with or without a threshold; a sequence line's '\r' asks none of its quality line
    short = c.records[0] + _record(b"short quality", b"ACGT" * 10, b"I" * 39)
    for kw in ({}, dict(min_qual_char="?")):
        with pytest.raises(ValueError, match="record 1: its quality line is shorter"):
            c.table.read_spans(dev(short), **kw)
    mixed = c.records[0] + b"@mixed\n" + b"ACGT" * 10 + b"\r\n+\n" + b"I" * 40 + b"\n"
    assert c.table.read_spans(dev(mixed)).cpu().numpy().tolist() == ref.read_spans(mixed, c.k, c.items).tolist()
    with pytest.raises(ValueError, match="upper"):
        c.table.read_spans(dev(good), lower=3, upper=2)
    with pytest.raises(ValueError, match="mode must be first or longest"):
        c.table.read_spans(dev(good), mode="last")
    assert c.unchanged()


# ------------------------------------------------------------------------------------------------------------ 2. trim_fastq

@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_trim_fastq_equals_the_reference(case, tmp_path):
    c = _corpus(case)
    for mode, min_len, form, pair in combos_of(c.kind, c.k):
        want = c.want(form, pair, mode, min_len)
        _in_band(want[2], f"{_IDS[CASES.index(case)]} {mode} min_len={min_len} {form} {pair}", second=c.k != 4)
        _same(_run(c, tmp_path, form, pair, mode, min_len), want)
    assert c.unchanged()
    assert sorted(os.listdir(tmp_path)) == sorted(n for n in os.listdir(tmp_path) if not n.endswith(".tmp"))


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[4], CASES[5]], ids=[_IDS[1], _IDS[2], _IDS[4], _IDS[5]])
def test_long_spans_leave_whole(case, tmp_path):
    """the window (0, 0), the absent k-mers: the foreign and poly structures are solid from end to end, so spans of 64 .. 5000
    positions, beginning at any offset of the line, go through the gather"""
    c = _corpus(case)
    for mode in MODES:
        for form, pair in (("interleaved", "single"), ("r1r2", "both")):
            want = c.want(form, pair, mode, c.k, window=(0, 0))
            _in_band(want[2], f"{_IDS[CASES.index(case)]} (0, 0) {mode} {form} {pair}")
            _same(_run(c, tmp_path, form, pair, mode, c.k, window=(0, 0)), want)
    out = c.want("interleaved", "single", "longest", c.k, window=(0, 0))[0]
    assert b"@poly S5000\n" + b"A" * (5000 + c.k - 1) + b"\n" in out and b"@poly N S1500 N S100\n" + b"A" * (1500 + c.k - 1) + b"\n" in out
    assert c.unchanged()


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[5]], ids=[_IDS[1], _IDS[4], _IDS[5]])
def test_quality_threshold_and_strict_case(case, tmp_path):
    c = _corpus(case)
    for kw in (dict(min_qual_char="5"), dict(lowercase_is_base=False), dict(min_qual_char="J", lowercase_is_base=False)):
        for form, pair in (("interleaved", "single"), ("r1r2", "both")):
            if kw.get("min_qual_char") == "J":       # no base is left: no read has a span
                got = _run(c, tmp_path, form, pair, "longest", c.k, **kw)
                assert got[0] == b"" and got[2]["kept"] == 0 and got[2]["kmers"] == 0 and got[2]["records"] == len(c.records)
                continue
            want = c.want(form, pair, "longest", c.k, **kw)
            _in_band(want[2], f"{_IDS[CASES.index(case)]} {kw} {form} {pair}")
            _same(_run(c, tmp_path, form, pair, "longest", c.k, **kw), want)
    assert c.want("interleaved", "single", "longest", c.k, min_qual_char="5")[0] != c.want("interleaved", "single", "longest", c.k)[0]
    assert c.want("interleaved", "single", "longest", c.k, lowercase_is_base=False)[0] != c.want("interleaved", "single", "longest", c.k)[0]
    assert c.unchanged()


@pytest.mark.parametrize("piece", [700, 4096])
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5]], ids=[_IDS[0], _IDS[3], _IDS[5]])
def test_pieces_give_the_one_piece_answer(case, piece, tmp_path, monkeypatch):
    c = _corpus(case)
    assert max(len(r) for r in c.records) > 2 * 4096 and min(len(r) for r in c.records) < 64     # a record beyond a piece; many to a piece
    mode, min_len = ("first", 4) if c.k == 4 else ("longest", c.k)
    whole = {f: _run(c, tmp_path, f, "both", mode, min_len, tag="whole") for f in ("interleaved", "r1r2")}
    monkeypatch.setenv("PG_FILTER_PIECE_BYTES", str(piece))
    for form in ("interleaved", "r1r2"):
        got = _run(c, tmp_path, form, "both", mode, min_len, tag="pieces")
        assert got[:2] == whole[form][:2]
        assert {n: v for n, v in got[2].items() if n not in ("seconds", "device_ms")} == {n: v for n, v in whole[form][2].items() if n not in ("seconds", "device_ms")}
        _same(got, c.want(form, "both", mode, min_len))
    assert c.unchanged()


@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=[_IDS[1], _IDS[3]])
def test_crlf_no_final_newline_and_gzip_give_the_same_records(case, tmp_path):
    c = _corpus(case)
    k = c.k
    kw = dict(lower=c.window[0], upper=c.window[1], mode="longest", min_len=k, pair="both")
    want = c.want("interleaved", "both", "longest", k)
    # CRLF: '\r' is a byte of its line and no base; every cut line keeps it.  The same records, the same spans
    crlf = b"".join(r.replace(b"\n", b"\r\n") for r in c.records)
    got = _run(c, tmp_path, "interleaved", "both", "longest", k, tag="crlf", data=crlf)
    _same(got, ref.trim_fastq(crlf, k, c.items, **kw))
    assert got[0].replace(b"\r\n", b"\n") == want[0] and got[0].count(b"\r\n") == got[0].count(b"\n") == 4 * want[2]["kept"]
    assert {n: got[2][n] for n in ("kept", "passed", "kmers", "hits", "bases_out")} == {n: want[2][n] for n in ("kept", "passed", "kmers", "hits", "bases_out")}
    # no final newline: the last record (kept: a pair that passes is appended) is written without one
    rows = ref.read_spans(c.data, k, c.items, *c.window, cache=c.cache)
    ok = (rows[:, 3] >= k).reshape(-1, 2).all(1)
    i = 2 * int(np.nonzero(ok)[0][0])
    for recs in (c.records, c.records + [c.records[i], c.records[i + 1]]):
        data = b"".join(recs)[:-1]
        got = _run(c, tmp_path, "interleaved", "both", "longest", k, tag="nonl", data=data)
        _same(got, ref.trim_fastq(data, k, c.items, **kw))
    assert got[0][-1:] != b"\n" and got[0].endswith(ref.trimmed_record(ref.records_of(c.records[i + 1][:-1])[0], *rows[i + 1, 2:].tolist()))
    # gzip input, one file and two
    src = tmp_path / "reads.fq.gz"
    src.write_bytes(gzip.compress(c.data))
    out = tmp_path / "from_gz.fq"
    res = c.table.trim_fastq(str(src), str(out), **kw)
    _same((out.read_bytes(), None, res), want)
    s1, s2, o1, o2 = (tmp_path / n for n in ("r1.fq.gz", "r2.fq", "o1.fq", "o2.fq"))
    s1.write_bytes(gzip.compress(c.r1))
    s2.write_bytes(c.r2)
    res = c.table.trim_fastq(str(s1), str(o1), str(s2), str(o2), **dict(kw, pair="any", mode="first"))
    _same((o1.read_bytes(), o2.read_bytes(), res), c.want("r1r2", "any", "first", k))
    assert c.unchanged()


@pytest.mark.parametrize("piece", [None, 700])
def test_errors_name_the_record_and_leave_no_output(piece, tmp_path, monkeypatch):
    c = _corpus(CASES[4])
    if piece:
        monkeypatch.setenv("PG_FILTER_PIECE_BYTES", str(piece))
    recs = c.records
    r = 41
    assert recs[r][:1] == b"@" and b"\n+" in recs[r]
    cut = b"".join(recs[:r]) + recs[r][:recs[r].index(b"\n+") + 1] + b"+\n"      # lines 4r .. 4r + 2, then nothing
    no_at = b"".join(recs[:r]) + b"x" + recs[r][1:] + b"".join(recs[r + 1:])
    no_plus = b"".join(recs[:r]) + recs[r].replace(b"\n+", b"\n-", 1) + b"".join(recs[r + 1:])
    short_q = b"".join(recs[:r]) + _record(b"short", b"ACGT" * 20, b"I" * 79) + b"".join(recs[r + 1:])
    odd = b"".join(recs[:r])
    out = tmp_path / "out.fq"

    def refused(data, match, **kw):
        src = tmp_path / "in.fq"
        src.write_bytes(data)
        with pytest.raises(ValueError, match=match):
            c.table.trim_fastq(str(src), str(out), **kw)
        assert sorted(os.listdir(tmp_path)) == ["in.fq"]

    refused(cut, f"record {r}: the file ends inside it")
    refused(no_at, f"record {r}: its first line does not begin with '@'")
    refused(no_plus, f"record {r}: its third line does not begin with '\\+'")
    refused(short_q, f"record {r}: its quality line is shorter")                  # (with and without a threshold: the quality is cut too)
    refused(short_q, f"record {r}: its quality line is shorter", min_qual_char="?", pair="single")
    refused(odd, f"record {r - 1} has no mate", pair="any")
    refused(odd, f"record {r - 1} has no mate")
    src = tmp_path / "in.fq"
    src.write_bytes(odd)                             # an odd count is fine where every record is judged on its own
    assert c.table.trim_fastq(str(src), str(out), pair="single")["records"] == r
    os.remove(out)
    os.remove(src)
    # R1 / R2 of different length, either way round
    s1, s2, o1, o2 = (tmp_path / n for n in ("r1.fq", "r2.fq", "o1.fq", "o2.fq"))
    for a, b in ((c.r1, b"".join(recs[1::2][:-3])), (b"".join(recs[0::2][:-3]), c.r2)):
        s1.write_bytes(a)
        s2.write_bytes(b)
        with pytest.raises(ValueError, match="same number of records"):
            c.table.trim_fastq(str(s1), str(o1), str(s2), str(o2))
        assert sorted(os.listdir(tmp_path)) == ["r1.fq", "r2.fq"]
    # an output that asks for gzip, and arguments that make no sense: refused before anything is opened
    s1.write_bytes(c.data)
    for kw, match in ((dict(out1=str(tmp_path / "o.fq.gz")), "plain text"), (dict(out1=str(o1), pair="all"), "pair must be"),
                      (dict(out1=str(o1), min_len=0), "min_len"), (dict(out1=str(o1), min_len=2.5), "min_len"), (dict(out1=str(o1), mode="last"), "mode must be"),
                      (dict(out1=str(o1), src2=str(s2)), "go together"),
                      (dict(out1=str(s1)), "must differ"), (dict(out1=str(o1), src2=str(s2), out2=str(o1)), "must differ"),
                      (dict(out1=str(o1), src2=str(s2), out2=str(s1)), "must differ"), (dict(out1=str(o1), src2=str(s2), out2=str(o2), pair="single"), "ONE file"),
                      (dict(out1=str(o1), lower=3, upper=2), "upper"), (dict(out1=str(o1), min_qual_char="??"), "one character")):
        with pytest.raises(ValueError, match=match):
            c.table.trim_fastq(str(s1), **kw)
        assert sorted(os.listdir(tmp_path)) == ["r1.fq", "r2.fq"]
    with pytest.raises(OSError):
        c.table.trim_fastq(str(tmp_path / "not_there.fq"), str(o1))
    assert sorted(os.listdir(tmp_path)) == ["r1.fq", "r2.fq"]
    assert c.unchanged()


# ------------------------------------------------------------------------------------------------------------ 3. the tool

def _main(argv):
    try:
        return cli.main_kmer_table(argv)
    except SystemExit as e:
        return e.code


def test_kmer_table_trim_from_a_dump_and_from_the_reads_themselves(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    c = _corpus(CASES[3])
    k = c.k
    (tmp_path / "reads.fq").write_bytes(c.data)
    (tmp_path / "r1.fq").write_bytes(c.r1)
    (tmp_path / "r2.fq").write_bytes(c.r2)
    c.table.write_dump("table.dump")
    capsys.readouterr()
    # -g: the table of the dump; R1 / R2, the first run, 50 bases and more, both mates must pass (the default)
    assert _main(["trim", "-g", "table.dump", "-k", str(k), "-1", "r1.fq", "-2", "r2.fq", "-o", "o1.fq", "-o2", "o2.fq", "--mode", "first",
                  "--min-len", "50"]) == 0
    out = capsys.readouterr()
    lines = out.out.splitlines()
    assert len(lines) == 1 and out.err == ""
    _same(((tmp_path / "o1.fq").read_bytes(), (tmp_path / "o2.fq").read_bytes(), json.loads(lines[0])), c.want("r1r2", "both", "first", 50))
    # no table source: the table is counted from the reads themselves; k-mers seen once are the errors' (and the foreign reads')
    from oracle import oracle
    seqs = b"".join(r[1].upper() + b"N" for r in ref.records_of(c.data))         # (the tables count lower-case bases)
    codes, counts = oracle.Table(k, threads=4).count(seqs).items()
    own = (codes, counts.astype(np.int64))
    want = ref.trim_fastq(c.data, k, own, lower=2, pair="single")
    _in_band(want[2], "the reads' own table, lower = 2", second=False)       # (nearly every kept read holds a k-mer seen once: 93 % are cut)
    capsys.readouterr()
    assert _main(["trim", "-k", str(k), "-i", "reads.fq", "-o", "solid.fq", "-L", "2", "--pair", "single"]) == 0
    out = capsys.readouterr()
    assert len(out.out.splitlines()) == 1 and out.err == ""
    _same(((tmp_path / "solid.fq").read_bytes(), None, json.loads(out.out)), want)
    # exit 1 and a message: a missing input, a mode that is none, mates asked of a file that has none
    (tmp_path / "odd.fq").write_bytes(b"".join(c.records[:3]))
    before = sorted(os.listdir(tmp_path))
    for argv, text in ((["trim", "-g", "table.dump", "-k", str(k), "-i", "not_there.fq", "-o", "x.fq"], "not_there.fq"),
                       (["trim", "-g", "table.dump", "-k", str(k), "-i", "reads.fq", "-o", "x.fq", "--mode", "last"], "--mode"),
                       (["trim", "-g", "table.dump", "-k", str(k), "-i", "odd.fq", "-o", "x.fq"], "has no mate")):
        assert _main(argv) == 1
        out = capsys.readouterr()
        assert out.out == "" and out.err.startswith("kmer_table: ") and text in out.err
        assert sorted(os.listdir(tmp_path)) == before
    assert c.unchanged()
