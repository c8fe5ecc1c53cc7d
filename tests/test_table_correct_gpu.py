"""Single substitutions in the reads of a FASTQ file put right from a finished table: ``KmerTable.read_corrections`` /
``KmerTable.correct_fastq`` (pg_fastq_index, pg_table_correct_reads, pg_fastq_gather) and ``kmer_table correct`` -- what khmer,
Lighter, BFC and Musket do, beside the read set of scripts/low_abd_reads.sh:10 (extract_unmapped.cpp).

Everything is integers and bytes, compared exactly with tests/_correct_ref.py (a numpy restatement of the semantics in
include/pangaea_feat.h).  Two corpora per table of tests/test_table_filter_gpu.py's six cases:

  * the DESIGNED corpus: a seeded random genome (3 000 bases, 60 for the dense k = 4 table) that is read as a circle, a table of
    the case's kind and geometry that holds exactly its k-mers (the genome written twice, counted), and about 400 reads cut from
    it with planted substitutions.  For k >= 13 a random k-mer is in the table with a chance of 1e-4 and less, so the answer of
    every named record is known by construction (``test_the_designed_corrections_are_there``); for k = 4 chance hits rule and
    only the reference says what is right.
  * the REAL corpus of the filter tests (``_built(case)``): equality with the reference only.

THE BAND, asserted on the reference's own result so that no case passes by changing nothing or everything.  k >= 13: between
25 % and 75 % of the designed records have at least one correction, at least 10 candidates are left as ambiguous and at least
10 have no valid base.  k = 4: at least 20 corrections and at least 10 ambiguous candidates."""
import functools
import gzip
import json
import os

import numpy as np
import pytest
import torch

from pangaea_amd import cli
from pangaea_amd.reads import ReadStream

from . import _correct_ref as ref
from .test_table_filter_gpu import CASES, DEV, _IDS, _alloc, _built, _record, window_of

pytestmark = pytest.mark.gpu


def _other(base: int, step: int = 1) -> int:
    """another base than ``base`` (a byte of ACGT)"""
    return b"ACGT"[(b"ACGT".index(base) + step) % 4]


class _Designed:
    def __init__(self, case):
        kind, k, log2_slots, log2_bucket = case
        self.k, self.kind = k, kind
        self.genome, self.records, self.designed = reads_of(k, 900 + k + log2_slots)
        size = len(self.genome)
        stream = ReadStream.from_runs([("genome twice", self.genome + self.genome + b"N")], device=DEV)
        self.table = _alloc(kind, k, log2_slots, log2_bucket).count(stream)
        assert self.table.kind == kind
        self.clone = self.table.data.clone()
        codes, counts = self.table.items()
        self.items = (codes, counts.astype(np.int64))
        assert counts.sum() == 2 * size - k + 1
        self.cache = {}
        self.names = [r[1:r.index(b"\n")] for r in self.records]
        self.data = b"".join(self.records)
        self.r1, self.r2 = b"".join(self.records[0::2]), b"".join(self.records[1::2])

    def unchanged(self):
        return torch.equal(self.table.data, self.clone)

    def want(self, lower=1, upper=None, lowercase_is_base=True, min_qual_char=None, data=None):
        return ref.read_corrections(self.data if data is None else data, self.k, self.items, lower, upper, lowercase_is_base, min_qual_char,
                                    cache=self.cache)


def reads_of(k: int, seed: int) -> tuple:
    """(the genome, the records, designed: name -> (candidates, corrected, the sequence line afterwards or None)) of a designed
    corpus"""
    rng = np.random.RandomState(seed)

    def rand(n):
        return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))

    # the genome, with a planted SNP repeat: X a Y and X c Y, both flanks of k + 5
    size = 60 if k == 4 else 3000
    X, Y = rand(k + 5), rand(k + 5)
    fill = size - 2 * (2 * k + 11)
    genome = rand(fill // 2) + X + b"A" + Y + rand(fill - fill // 2) + X + b"C" + Y
    assert len(genome) == size
    snps = {fill // 2 + k + 5, size - (k + 5) - 1}
    assert {genome[s] for s in snps} == {ord("A"), ord("C")}
    circle = genome * (2 + 5000 // size + 1)

    def piece(n, avoid=()):
        """n bases of the circle that do not put a SNP site at one of the read positions ``avoid``"""
        while True:
            at = int(rng.randint(size))
            if not any((at + p) % size in snps for p in avoid):
                return bytearray(circle[at:at + n])

    recs, designed = [], {}                              # designed: name -> (candidates, corrected, the sequence line afterwards)

    def add(name, seq, want=None, qual=None):
        name = b"%s #%d" % (name, len(recs))
        recs.append(_record(name, bytes(seq), qual))
        if want is not None:
            designed[name] = want

    # 1. one error at every position that matters, in reads of every length that matters.  The k-mers that hold base p are
    # at [max(0, p - k + 1), min(p, n - k)]: a candidate unless they are all the read has
    for n in (k, k + 1, 2 * k - 1, 2 * k, 150, 700, 5000):
        for p in sorted({0, 1, k - 2, k - 1, k, 63, 64, 64 + k - 1, 511, 512, 512 + k - 2, n - k - 1, n - k, n - 1}):
            if not 0 <= p < n:
                continue
            good = piece(n, (p,))
            seq = bytearray(good)
            seq[p] = _other(good[p], 1 + p % 3)
            fixed = min(p, n - k) - max(0, p - k + 1) + 1 < n - k + 1
            add(b"one n=%d p=%d" % (n, p), seq, (1, 1, bytes(good)) if fixed else (0, 0, bytes(seq)))
    # 2. two errors d apart: closer than k + 1 they make one run of k + d, which is no candidate; k + 1 apart two runs of k
    for d in (1, k - 1, k, k + 1):
        for n, p in ((150, 60), (700, 500 - d), (5000, 512 - 1)):
            good = piece(n, (p, p + d))
            seq = bytearray(good)
            seq[p], seq[p + d] = _other(good[p]), _other(good[p + d], 2)
            add(b"two n=%d p=%d d=%d" % (n, p, d), seq, (2, 2, bytes(good)) if d == k + 1 else (0, 0, bytes(seq)))
    # 3. an error within k of an N; within k of a '#' (a base unless a threshold is asked); at a lower-case position
    for i, (p, gap) in enumerate(((75, 1), (75, k - 1), (75, -1), (75, -(k - 1)), (600, 2), (600, -2))):
        good = piece(700, (p,))
        seq = bytearray(good)
        seq[p] = _other(good[p])
        seq[p + gap] = ord("N")
        add(b"beside N p=%d gap=%d" % (p, gap), seq, (0, 0, bytes(seq)))
        seq = bytearray(good)
        seq[p] = _other(good[p])
        qual = bytearray(b"I" * 700)
        qual[p + gap] = ord("#")
        add(b"beside # p=%d gap=%d" % (p, gap), seq, (1, 1, bytes(good)), bytes(qual))
        good[p] |= 0x20
        seq = bytearray(good)
        seq[p] = _other(good[p] & 0xDF) | 0x20
        add(b"lower p=%d %d" % (p, i), seq, (1, 1, bytes(good)))
    # 4. reads that are wrong throughout, and reads without an error
    for i in range(8):
        add(b"all wrong %d" % i, rand(150), (0, 0, None))
    for n in (k, k + 1, 150, 150, 150, 700, 5000):
        good = piece(n)
        add(b"right n=%d" % n, good, (0, 0, bytes(good)))
    # 5. the planted SNP repeat: X g Y and X t Y fit both X a Y and X c Y (and nothing else) -- ambiguous
    for i in range(12):
        left, right = k + i % 6, k - 1 + (i // 2) % 6     # (a flank of k - 1 on both sides would leave no solid k-mer)
        seq = X[len(X) - left:] + (b"G" if i % 2 else b"T") + Y[:right]
        add(b"snp %d" % i, seq, (1, 0, seq))
    # 6. candidates without a valid base: two unrelated pieces with one base between them (k k-mers hold it, and no base there
    # joins the pieces), and a read with two or three foreign bases at its end
    for i in range(8):
        at_a, at_b = int(rng.randint(size)), size + int(rng.randint(size))
        between = [c for c in b"ACGT" if c not in (circle[at_a + 60 + i], circle[at_b - 1])][0]      # (it continues neither piece)
        seq = circle[at_a:at_a + 60 + i] + bytes([between]) + circle[at_b:at_b + 70]
        add(b"joint %d" % i, seq, (1, 0, seq))
    for i in range(6):
        good = piece(100 + i)
        seq = bytes(good) + rand(2 + i % 2)
        add(b"tail %d" % i, seq, None)                   # (the foreign bases are random: what they are is the reference's to say)
    # 7. reads of the usual length with zero to three errors anywhere, N's among them: the reference's to say
    while len(recs) < 400:
        seq = piece(150)
        for _ in range(int(rng.randint(4))):
            p = int(rng.randint(150))
            seq[p] = rng.choice([c for c in b"ACGTN" if c != seq[p]])
        qual = np.full(150, ord("I"), np.uint8)
        if rng.rand() < 0.3:
            qual[rng.rand(150) < 0.05] = ord("#")
        add(b"any", seq, None, bytes(qual))
    return genome, recs, designed


@functools.lru_cache(maxsize=None)
def _designed(case):
    return _Designed(case)


def _dev(data: bytes) -> torch.Tensor:
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)


def _seq_lines(data: bytes) -> list:
    return data.split(b"\n")[1::4]


# ------------------------------------------------------------------------------------------------------------ 1. the corpus

@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_the_designed_corrections_are_there(case):
    """the reference alone, record by record: every named record gives what it was designed to give (k >= 13), and the band"""
    c = _designed(case)
    k = c.k
    assert 400 <= len(c.records) <= 420
    rows, out, gained, details = c.want()
    lines = _seq_lines(out)
    if k >= 13:
        for name, (candidates, corrected, after) in c.designed.items():
            r = c.names.index(name)
            assert rows[r, 2:].tolist() == [candidates, corrected], (name, rows[r], details[r])
            assert after is None or lines[r] == after, name
        # the strict case leaves the lower-case errors alone, a threshold those beside a '#'
        strict, quality = c.want(lowercase_is_base=False)[0], c.want(min_qual_char="5")[0]
        for name in c.designed:
            r = c.names.index(name)
            if name.startswith(b"lower"):
                assert strict[r, 2:].tolist() == [0, 0], name
            if name.startswith(b"beside #"):
                assert quality[r, 2:].tolist() == [0, 0] and rows[r, 2:].tolist() == [1, 1], name
        named = np.array([n in c.designed for n in c.names])
        share = float((rows[named, 3] > 0).mean())
        valid = [len(v) for d in details for *_, v in d]
        print(f"k={k}: {share:.3f} of {named.sum()} designed records corrected; ambiguous {sum(v > 1 for v in valid)}, no valid base {valid.count(0)}")
        assert 0.25 <= share <= 0.75
        assert sum(v > 1 for v in valid) >= 10 and valid.count(0) >= 10
    else:
        valid = [len(v) for d in details for *_, v in d]
        print(f"k={k}: corrected {valid.count(1)}, ambiguous {sum(v > 1 for v in valid)}, no valid base {valid.count(0)}")
        assert valid.count(1) >= 20 and sum(v > 1 for v in valid) >= 10
    # the shapes the kernel can go wrong at are in the corpus: runs that close in the next ballot word, in the next batch, and a
    # window that begins in the batch before
    closes = {(a // 64, b // 64, a // 512, b // 512) for d in details for a, b, *_ in d}
    assert any(wa != wb for wa, wb, _, _ in closes) and any(ba != bb for _, _, ba, bb in closes)


# ------------------------------------------------------------------------------------------------------------ 2. read_corrections

def _equal(c, data, text, lower, upper, lenient=True, mq=None):
    got_rows, got_text = c.table.read_corrections(text, lower=lower, upper=upper, lowercase_is_base=lenient, min_qual_char=mq)
    rows, out, gained, _ = ref.read_corrections(data, c.k, c.items, lower, upper, lenient, mq, cache=c.cache)
    assert got_rows.dtype == torch.int64 and got_rows.device == text.device and got_rows.shape == rows.shape
    assert got_text.dtype == torch.uint8 and got_text.device == text.device and got_text.shape == text.shape
    bad = np.nonzero((got_rows.cpu().numpy() != rows).any(1))[0]
    assert len(bad) == 0, (lower, upper, lenient, mq, bad[:5], got_rows[bad[:5]], rows[bad[:5]])
    fixed = got_text.cpu().numpy().tobytes()
    if fixed != out:
        at = int(np.nonzero(np.frombuffer(fixed, np.uint8) != np.frombuffer(out, np.uint8))[0][0])
        raise AssertionError((lower, upper, lenient, mq, at, fixed[max(0, at - 40):at + 40], out[max(0, at - 40):at + 40]))
    return rows, out, gained, got_rows, got_text


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_read_corrections_of_the_designed_corpus(case):
    c = _designed(case)
    text = _dev(c.data)
    before = text.clone()
    asked = [(1, None, True, None), (2, 5, True, None), (0, 0, True, None), (1, None, False, None), (1, None, True, "5")]
    seen = set()
    for lower, upper, lenient, mq in asked:
        rows, out, gained, got_rows, got_text = _equal(c, c.data, text, lower, upper, lenient, mq)
        seen.add(rows.tobytes())
        assert torch.equal(text, before)                     # (the argument is not modified)
        # h has grown by the corrected runs' lengths, and a second call corrects nothing
        kw = dict(lower=lower, upper=upper, lowercase_is_base=lenient, min_qual_char=mq)
        hits = c.table.read_hits(got_text, **kw)
        assert torch.equal(hits[:, 0], got_rows[:, 0]) and hits[:, 1].cpu().numpy().tolist() == (rows[:, 1] + gained).tolist()
        assert torch.equal(c.table.read_hits(text, **kw), got_rows[:, :2])
        again, same = c.table.read_corrections(got_text, **kw)
        assert torch.equal(same, got_text) and not again[:, 3].any()
        assert torch.equal(again[:, 2], got_rows[:, 2] - got_rows[:, 3]) and torch.equal(again[:, :2], hits)
    assert len(seen) >= 4                                # (the windows and rules ask different questions of this corpus)
    # a view that does not begin at a 16-byte boundary; nothing at all
    off = torch.cat([torch.zeros(3, dtype=torch.uint8, device=DEV), text])[3:]
    for a, b in zip(c.table.read_corrections(off), c.table.read_corrections(text)):
        assert torch.equal(a, b)
    rows, fixed = c.table.read_corrections(text[:0])
    assert rows.shape == (0, 4) and rows.dtype == torch.int64 and fixed.shape == (0,) and fixed.dtype == torch.uint8
    assert c.unchanged()


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_read_corrections_of_the_real_corpus(case):
    b = _built(case)

    class Real:
        k, items, table, cache = b.k, b.items, b.table, {}

    text = _dev(b.data)
    for lower, upper in ((2, None), (1, None), window_of(b.k, b.items)):
        _equal(Real, b.data, text, lower, upper)
    assert b.unchanged()


def test_read_corrections_refuses_a_cpu_tensor_and_malformed_text():
    c = _designed(CASES[1])
    good = c.records[0] + c.records[1]
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        c.table.read_corrections(torch.frombuffer(bytearray(good), dtype=torch.uint8))
    assert c.table.read_corrections(_dev(good))[0].shape == (2, 4)
    for data, record in ((good[:-5].rsplit(b"\n", 1)[0], 1), (good + b"\n", 2), (b"\n", 0), (good.replace(b"@", b"", 1), 0),
                         (c.records[0] + c.records[1].replace(b"\n+", b"\n-", 1) + c.records[2], 1)):
        with pytest.raises(ValueError, match=f"record {record}:"):
            c.table.read_corrections(_dev(data))
    short = c.records[0] + _record(b"short quality", b"ACGT" * 10, b"I" * 39)
    for kw in ({}, dict(min_qual_char="?")):
        with pytest.raises(ValueError, match="record 1: its quality line is shorter"):
            c.table.read_corrections(_dev(short), **kw)
    # a sequence line's '\r' asks none of its quality line; CRLF: the error at the right end is corrected
    i = c.names.index([n for n in c.names if n.startswith(b"one n=150 p=149")][0])
    mixed = c.records[0] + c.records[i].replace(b"\n+", b"\r\n+", 1)
    crlf = c.records[i].replace(b"\n", b"\r\n") + c.records[0]
    for data in (mixed, crlf):
        rows, out, _, _ = ref.read_corrections(data, c.k, c.items)
        got_rows, got_text = c.table.read_corrections(_dev(data))
        assert got_rows.cpu().numpy().tolist() == rows.tolist() and got_text.cpu().numpy().tobytes() == out
        assert rows[:, 3].sum() == 1 and out != data
    with pytest.raises(ValueError, match="upper"):
        c.table.read_corrections(_dev(good), lower=3, upper=2)
    with pytest.raises(TypeError):
        c.table.read_corrections(_dev(good).to(torch.int32))
    assert c.unchanged()


# ------------------------------------------------------------------------------------------------------------ 3. correct_fastq

_TOTALS = ("records", "bases", "kmers", "hits", "candidates", "corrected", "reads_corrected")


def _run(c, tmp_path, form, tag="x", data=None, **kw):
    """(bytes written 1, bytes written 2 or None, the returned dict) of ``correct_fastq`` on files written for the call"""
    if form == "interleaved":
        src = tmp_path / f"{tag}.fq"
        src.write_bytes(c.data if data is None else data)
        out = tmp_path / f"{tag}.out.fq"
        res = c.table.correct_fastq(str(src), str(out), **kw)
        assert os.path.getsize(out) == os.path.getsize(src)
        return out.read_bytes(), None, res
    s1, s2, o1, o2 = (tmp_path / f"{tag}.{n}.fq" for n in ("r1", "r2", "o1", "o2"))
    s1.write_bytes(c.r1 if data is None else data[0])
    s2.write_bytes(c.r2 if data is None else data[1])
    res = c.table.correct_fastq(str(s1), str(o1), str(s2), str(o2), **kw)
    assert os.path.getsize(o1) == os.path.getsize(s1) and os.path.getsize(o2) == os.path.getsize(s2)
    return o1.read_bytes(), o2.read_bytes(), res


def _same(got, want):
    g1, g2, res = got
    w1, w2, tot = want
    assert g1 == w1 and g2 == w2
    assert tuple(tot) == _TOTALS and {n: res[n] for n in tot} == tot
    assert set(res) == set(tot) | {"seconds", "device_ms"} and res["seconds"] > 0 and res["device_ms"] >= 0
    for n in tot:
        assert type(res[n]) is int


def _differs_in_the_corrected_bases(src: bytes, out: bytes, corrected: int):
    assert len(src) == len(out)
    at = np.nonzero(np.frombuffer(src, np.uint8) != np.frombuffer(out, np.uint8))[0]
    assert len(at) == corrected
    line = np.concatenate([[0], np.cumsum(np.frombuffer(src, np.uint8) == 10)])[at]          # (the line every changed byte is on)
    assert (line % 4 == 1).all()


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_correct_fastq_equals_the_reference(case, tmp_path):
    c = _designed(case)
    for kw in (dict(), dict(lower=2, upper=5), dict(min_qual_char="5"), dict(lowercase_is_base=False)):
        for form in ("interleaved", "r1r2"):
            a, b = (c.data, None) if form == "interleaved" else (c.r1, c.r2)
            want = ref.correct_fastq(a, c.k, c.items, b, cache=c.cache, **kw)
            got = _run(c, tmp_path, form, **kw)
            _same(got, want)
            srcs = [a] if b is None else [a, b]
            changed = sum(int((np.frombuffer(s, np.uint8) != np.frombuffer(o, np.uint8)).sum()) for s, o in zip(srcs, got[:2]))
            assert changed == want[2]["corrected"]
            if b is None:
                _differs_in_the_corrected_bases(a, got[0], want[2]["corrected"])
    assert ref.correct_fastq(c.data, c.k, c.items, cache=c.cache)[2]["corrected"] >= 20
    assert c.unchanged()
    assert sorted(os.listdir(tmp_path)) == sorted(n for n in os.listdir(tmp_path) if not n.endswith(".tmp"))


@pytest.mark.parametrize("piece", [700, 4096])
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5]], ids=[_IDS[0], _IDS[3], _IDS[5]])
def test_pieces_give_the_one_piece_answer(case, piece, tmp_path, monkeypatch):
    c = _designed(case)
    assert max(len(r) for r in c.records) > 2 * 4096 and min(len(r) for r in c.records) < 100     # a record beyond a piece; many to a piece
    whole = {f: _run(c, tmp_path, f, tag="whole") for f in ("interleaved", "r1r2")}
    monkeypatch.setenv("PG_FILTER_PIECE_BYTES", str(piece))
    for form in ("interleaved", "r1r2"):
        got = _run(c, tmp_path, form, tag="pieces")
        assert got[:2] == whole[form][:2]
        assert {n: got[2][n] for n in _TOTALS} == {n: whole[form][2][n] for n in _TOTALS}
        a, b = (c.data, None) if form == "interleaved" else (c.r1, c.r2)
        _same(got, ref.correct_fastq(a, c.k, c.items, b, cache=c.cache))
    assert c.unchanged()


@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=[_IDS[1], _IDS[3]])
def test_crlf_no_final_newline_and_gzip_give_the_same_corrections(case, tmp_path):
    c = _designed(case)
    k = c.k
    want = ref.correct_fastq(c.data, k, c.items, cache=c.cache)
    # CRLF: the '\r' is beyond the end of the bases, so the right-end errors are corrected as they are without it
    crlf = b"".join(r.replace(b"\n", b"\r\n") for r in c.records)
    got = _run(c, tmp_path, "interleaved", tag="crlf", data=crlf)
    _same(got, ref.correct_fastq(crlf, k, c.items))
    assert got[0].replace(b"\r\n", b"\n") == want[0]
    assert {n: got[2][n] for n in _TOTALS[2:]} == {n: want[2][n] for n in _TOTALS[2:]} and got[2]["bases"] == want[2]["bases"] + len(c.records)
    _differs_in_the_corrected_bases(crlf, got[0], want[2]["corrected"])
    # no final newline, and an odd number of records: one file needs no mates
    i = c.names.index([n for n in c.names if n.startswith(b"one n=150 p=149")][0])
    for recs in (c.records, c.records + [c.records[i]]):
        data = b"".join(recs)[:-1]
        got = _run(c, tmp_path, "interleaved", tag="nonl", data=data)
        _same(got, ref.correct_fastq(data, k, c.items))
    assert got[0][-1:] != b"\n" and got[2]["records"] == len(c.records) + 1 and got[0] != data
    # gzip input, one file and two
    src = tmp_path / "reads.fq.gz"
    src.write_bytes(gzip.compress(c.data))
    out = tmp_path / "from_gz.fq"
    res = c.table.correct_fastq(str(src), str(out))
    _same((out.read_bytes(), None, res), want)
    s1, s2, o1, o2 = (tmp_path / n for n in ("r1.fq.gz", "r2.fq", "o1.fq", "o2.fq"))
    s1.write_bytes(gzip.compress(c.r1))
    s2.write_bytes(c.r2)
    res = c.table.correct_fastq(str(s1), str(o1), str(s2), str(o2))
    _same((o1.read_bytes(), o2.read_bytes(), res), ref.correct_fastq(c.r1, k, c.items, c.r2, cache=c.cache))
    assert c.unchanged()


@pytest.mark.parametrize("piece", [None, 700])
def test_errors_name_the_record_and_leave_no_output(piece, tmp_path, monkeypatch):
    c = _designed(CASES[4])
    if piece:
        monkeypatch.setenv("PG_FILTER_PIECE_BYTES", str(piece))
    recs = c.records
    r = 41
    assert recs[r][:1] == b"@" and b"\n+" in recs[r]
    cut = b"".join(recs[:r]) + recs[r][:recs[r].index(b"\n+") + 1] + b"+\n"      # lines 4r .. 4r + 2, then nothing
    no_at = b"".join(recs[:r]) + b"x" + recs[r][1:] + b"".join(recs[r + 1:])
    no_plus = b"".join(recs[:r]) + recs[r].replace(b"\n+", b"\n-", 1) + b"".join(recs[r + 1:])
    short_q = b"".join(recs[:r]) + _record(b"short", b"ACGT" * 20, b"I" * 79) + b"".join(recs[r + 1:])
    out = tmp_path / "out.fq"

    def refused(data, match, **kw):
        src = tmp_path / "in.fq"
        src.write_bytes(data)
        with pytest.raises(ValueError, match=match):
            c.table.correct_fastq(str(src), str(out), **kw)
        assert sorted(os.listdir(tmp_path)) == ["in.fq"]

    refused(cut, f"record {r}: the file ends inside it")
    refused(no_at, f"record {r}: its first line does not begin with '@'")
    refused(no_plus, f"record {r}: its third line does not begin with '\\+'")
    refused(short_q, f"record {r}: its quality line is shorter")
    refused(short_q, f"record {r}: its quality line is shorter", min_qual_char="?")
    os.remove(tmp_path / "in.fq")
    # R1 / R2 of different length, either way round
    s1, s2, o1, o2 = (tmp_path / n for n in ("r1.fq", "r2.fq", "o1.fq", "o2.fq"))
    for a, b in ((c.r1, b"".join(recs[1::2][:-3])), (b"".join(recs[0::2][:-3]), c.r2)):
        s1.write_bytes(a)
        s2.write_bytes(b)
        with pytest.raises(ValueError, match="same number of records"):
            c.table.correct_fastq(str(s1), str(o1), str(s2), str(o2))
        assert sorted(os.listdir(tmp_path)) == ["r1.fq", "r2.fq"]
    # an output that asks for gzip, and arguments that make no sense: refused before anything is opened
    s1.write_bytes(c.data)
    for kw, match in ((dict(out1=str(tmp_path / "o.fq.gz")), "plain text"), (dict(out1=str(o1), src2=str(s2)), "go together"),
                      (dict(out1=str(s1)), "must differ"), (dict(out1=str(o1), src2=str(s2), out2=str(o1)), "must differ"),
                      (dict(out1=str(o1), src2=str(s2), out2=str(s1)), "must differ"),
                      (dict(out1=str(o1), lower=3, upper=2), "upper"), (dict(out1=str(o1), lower=-1), "lower"),
                      (dict(out1=str(o1), min_qual_char="??"), "one character")):
        with pytest.raises(ValueError, match=match):
            c.table.correct_fastq(str(s1), **kw)
        assert sorted(os.listdir(tmp_path)) == ["r1.fq", "r2.fq"]
    with pytest.raises(OSError):
        c.table.correct_fastq(str(tmp_path / "not_there.fq"), str(o1))
    assert sorted(os.listdir(tmp_path)) == ["r1.fq", "r2.fq"]
    assert c.unchanged()


# ------------------------------------------------------------------------------------------------------------ 4. the tool

def _main(argv):
    try:
        return cli.main_kmer_table(argv)
    except SystemExit as e:
        return e.code


def test_kmer_table_correct_from_a_dump_and_from_the_reads_themselves(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    c = _designed(CASES[3])
    k = c.k
    (tmp_path / "reads.fq").write_bytes(c.data)
    (tmp_path / "r1.fq").write_bytes(c.r1)
    (tmp_path / "r2.fq").write_bytes(c.r2)
    c.table.write_dump("table.dump")
    capsys.readouterr()
    # -g: the table of the dump; R1 / R2
    assert _main(["correct", "-g", "table.dump", "-k", str(k), "-1", "r1.fq", "-2", "r2.fq", "-o", "o1.fq", "-o2", "o2.fq"]) == 0
    out = capsys.readouterr()
    lines = out.out.splitlines()
    assert len(lines) == 1 and out.err == ""
    _same(((tmp_path / "o1.fq").read_bytes(), (tmp_path / "o2.fq").read_bytes(), json.loads(lines[0])),
          ref.correct_fastq(c.r1, k, c.items, c.r2, cache=c.cache))
    # no table source: the table is counted from the reads themselves, where a k-mer seen once is an error's: -L 2
    from oracle import oracle
    from ._trim_ref import records_of
    seqs = b"".join(r[1].upper() + b"N" for r in records_of(c.data))             # (the tables count lower-case bases)
    codes, counts = oracle.Table(k, threads=4).count(seqs).items()
    own = (codes, counts.astype(np.int64))
    want = ref.correct_fastq(c.data, k, own, lower=2)
    assert want[2]["corrected"] >= 1 and want[0] != c.data
    capsys.readouterr()
    assert _main(["correct", "-k", str(k), "-i", "reads.fq", "-o", "fixed.fq", "-L", "2"]) == 0
    out = capsys.readouterr()
    assert len(out.out.splitlines()) == 1 and out.err == ""
    _same(((tmp_path / "fixed.fq").read_bytes(), None, json.loads(out.out)), want)
    # exit 1 and a message: a missing input, a window that is none, a file that ends inside a record
    (tmp_path / "cut.fq").write_bytes(c.data[:len(c.data) - len(c.records[-1]) + 10])
    before = sorted(os.listdir(tmp_path))
    for argv, text in ((["correct", "-g", "table.dump", "-k", str(k), "-i", "not_there.fq", "-o", "x.fq"], "not_there.fq"),
                       (["correct", "-g", "table.dump", "-k", str(k), "-i", "reads.fq", "-o", "x.fq", "-L", "3", "-U", "2"], "-U"),
                       (["correct", "-g", "table.dump", "-k", str(k), "-i", "cut.fq", "-o", "x.fq"], "the file ends inside it")):
        assert _main(argv) == 1
        out = capsys.readouterr()
        assert out.out == "" and out.err.startswith("kmer_table: ") and text in out.err
        assert sorted(os.listdir(tmp_path)) == before
    assert c.unchanged()
