"""Reads of a FASTQ file kept or dropped by the counts of their k-mers in a finished table: ``KmerTable.read_hits`` /
``KmerTable.filter_fastq`` (pg_fastq_index, pg_table_read_hits, pg_fastq_gather) and ``kmer_table filter`` -- what `kmc_tools filter`
does, beside the read set of scripts/low_abd_reads.sh:10 (extract_unmapped.cpp).

Everything is integers and bytes, compared exactly with tests/_filter_ref.py (a numpy restatement of the semantics in
include/pangaea_feat.h).  One table per kind at the edges of its k range, one corpus and one set of reference counts per table,
shared by the tests; every table is cloned when it is built and compared with its clone after each test.

THE BAND.  Every ``filter_fastq`` case is asserted, on the reference's own result, to keep between 10 % and 90 % of the records,
so that no case passes by keeping everything or nothing.  Of the 5 x 3 combinations of ``min_hits`` in {1, 3, 0.0, 0.5, 1.0} and
``max_hits`` in {None, 0, 0.25} the following are left out, for every table, pair rule and input form, because the reference
itself is outside the band there (the rule, then what it leaves out):
  * ``max_hits`` below a ``min_hits`` it cannot meet keeps nothing: (1, 0), (3, 0), (0.5, 0), (1.0, 0), (0.5, 0.25), (1.0, 0.25);
  * (0.0, None) keeps every read that has a k-mer: more than 90 %.
What stays -- (1, None), (3, None), (0.5, None), (1.0, None), (0.0, 0), (0.0, 0.25), (1, 0.25), (3, 0.25); the last two cut between
reads that HAVE hits, which is what the corpus' 60 reads of k + 9 own characters are for -- is in the band for every table, rule
and form, with two exceptions (``combos_of``):
  * the mini k = 13 table: a random 13-mer is in the table by chance often enough (one in a few hundred) that a good part of
    the foreign reads have a hit.  (0.0, 0) then keeps 9.5 % under ``both``, and (1, None) 89.9 % under ``any``: both are left out
    for that table -- (0.0, 0.25) and (3, None) ask the same two questions inside the band;
  * the dense k = 4 table.  Its 256 counters are all far above 0, so its window is retuned to [the count that half of the
    table's OCCURRENCES reach, no upper bound]: about half of any read's 4-mers are hits then, whatever genome it came from, and
    ``min_hits = 0.5`` splits the reads near the middle.  No other combination can tell reads apart by a table of 4-mers (every
    read has hits, none has only hits, none has under a quarter): for that table (0.5, None) alone is run."""
import functools
import gzip
import json
import os

import numpy as np
import pytest
import torch

from pangaea_amd import cli, kmer, synth

from . import _filter_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (kind, k, log2_slots, log2_bucket): every kind at an edge of its k range, one table of a single bucket
CASES = [("dense", 4, 0, 0), ("hash", 21, 20, 10), ("wide", 31, 20, 0), ("mini", 13, 18, 12), ("mini", 21, 14, 14), ("miniw", 22, 20, 13)]
_IDS = [f"{c[0]}-k{c[1]}-s{c[2]}-b{c[3]}" for c in CASES]
WINDOWS = [(1, None), (2, 5), (1, 1), (0, 0)]
_KEPT = [(1, None), (3, None), (0.5, None), (1.0, None), (0.0, 0), (0.0, 0.25), (1, 0.25), (3, 0.25)]
_KEPT_DENSE4 = [(0.5, None)]
FORMS = [("interleaved", "any"), ("interleaved", "both"), ("interleaved", "single"), ("r1r2", "any"), ("r1r2", "both")]


def _synth_cfg(k, log2_slots):
    if log2_slots == 14:
        return synth.SynthConfig(n_pairs=40, n_barcodes=2, n_genomes=3, genome_len=30_000, fragment=8_000, sub_rate=0.01, n_rate=0.2, seed=700 + k)
    return synth.SynthConfig(n_pairs=1000, n_barcodes=37, n_genomes=3, genome_len=30_000, fragment=8_000, sub_rate=0.01, n_rate=0.2, seed=700 + k)


def _alloc(kind, k, log2_slots, log2_bucket):
    if kind == "dense":
        return kmer.KmerTable.alloc(k, DEV, "dense")
    if kind == "hash":
        return kmer.KmerTable.with_slots(k, DEV, log2_slots, log2_bucket)
    if kind == "wide":
        return kmer.KmerTable.wide_with_slots(k, DEV, log2_slots)
    return kmer.KmerTable.mini_with_slots(k, DEV, log2_slots, log2_bucket)


def _record(name: bytes, seq: bytes, qual: bytes = None, plus: bytes = b"+") -> bytes:
    return b"@" + name + b"\n" + seq + b"\n" + plus + b"\n" + (b"I" * len(seq) if qual is None else qual) + b"\n"


def corpus_of(text: bytes, n_pairs: int, k: int, seed: int) -> list:
    """about 360 records, mates next to each other: reads of the table's own text (302 characters per pair: read, N, read, N),
    as many of a genome it never saw, chimeras of half each, mostly paired with their own kind, 30 pairs of reads with a few
    hits only (so that an upper bound of a quarter cuts between reads that have hits); then the hand-made edge records"""
    rng = np.random.RandomState(seed)

    def own(n=150):
        p = int(rng.randint(n_pairs))
        return text[302 * p:302 * p + 150][:n]

    def foreign(n=150):
        return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))

    def chimera():
        return own(75) + foreign(75)

    def mostly_foreign():                            # k + 9 characters of the table's text: 10 hits, well under a quarter of the k-mers
        return own(k + 9) + foreign(150 - (k + 9))

    def quality(seq):
        q = np.full(len(seq), ord("I"), np.uint8)
        if rng.rand() < 0.3:
            q[rng.rand(len(seq)) < 0.1] = ord("#")
        return bytes(q)

    recs = []
    kinds = [(own, own)] * 38 + [(foreign, foreign)] * 38 + [(chimera, chimera)] * 38 + [(own, foreign)] * 8 + [(foreign, chimera)] * 8 + [(chimera, own)] * 8
    kinds += [(mostly_foreign, mostly_foreign)] * 30
    for i in rng.permutation(len(kinds)):
        for m, make in enumerate(kinds[i]):
            seq = make()
            name = b"r%d/%d" % (i, m + 1) if i % 3 else b"r%d\tBX:Z:ACGTACGTACGTACGT-1\tQX:Z:IIII" % i if i % 2 else b"r%d BX:Z:TTTT-1 mate %d" % (i, m + 1)
            recs.append(_record(name, seq, quality(seq), b"+" + name if i % 5 == 0 else b"+"))
    clean = text.replace(b"N", b"")
    at = [0]

    def stretch(n):                                  # n characters of the table's text without its separators, then foreign ones
        a = at[0]
        at[0] += n
        s = clean[a:a + n]
        return s + foreign(n - len(s))

    edges = [b"", b"A", stretch(k - 1), stretch(k), stretch(k + 1)]
    edges += [stretch(n_pos + k - 1) for n_pos in (63, 64, 65, 511, 512, 513, 1500, 5000)]
    r = own().replace(b"N", b"A")
    edges += [b"N" + r[1:], r[:-1] + b"N", r[:75] + b"N" + r[76:], b"N" * 150, r.lower(), foreign().lower()]
    for i, seq in enumerate(edges):
        recs.append(_record(b"edge%d len=%d" % (i, len(seq)), seq))
    r = own()
    recs.append(_record(b"quality begins with @", r, b"@" + b"I" * (len(r) - 1)))
    recs.append(_record(b"quality begins with +", r, b"+" + b"#" * (len(r) - 1), b"+quality begins with +"))
    recs.append(_record(b"long quality", r[:100], b"I" * 120))
    if len(recs) % 2:
        recs.append(_record(b"the last one's mate", foreign()))
    return recs


def window_of(k: int, items) -> tuple:
    """the count window of the ``filter_fastq`` cases: [1, none] -- but every 4-mer is in a table of real reads, so there [the count
    that half of the table's occurrences reach, none] (the module's docstring)"""
    if k != 4:
        return 1, None
    c = np.sort(items[1])
    total = np.cumsum(c)
    return int(c[np.searchsorted(total, total[-1] / 2)]), None


def combos_of(k: int) -> list:
    """the (min_hits, max_hits) cases of a table (the module's docstring says which are left out, and why)"""
    if k == 4:
        return _KEPT_DENSE4
    return [c for c in _KEPT if c not in ((0.0, 0), (1, None))] if k == 13 else _KEPT


class _Built:
    def __init__(self, case):
        kind, k, log2_slots, log2_bucket = case
        cfg = _synth_cfg(k, log2_slots)
        reads = synth.generate(cfg, device=DEV)
        self.k, self.kind = k, kind
        self.table = _alloc(kind, k, log2_slots, log2_bucket).count(reads)
        assert self.table.kind == kind
        self.clone = self.table.data.clone()
        text = reads.decode()
        assert len(text) == 302 * cfg.n_pairs
        codes, counts = self.table.items()
        self.items = (codes, counts.astype(np.int64))
        self.records = corpus_of(text, cfg.n_pairs, k, 800 + k)
        self.data = b"".join(self.records)
        self.r1, self.r2 = b"".join(self.records[0::2]), b"".join(self.records[1::2])
        self.window = window_of(k, self.items)
        self.cache = {}

    def unchanged(self):
        return torch.equal(self.table.data, self.clone)

    def want(self, form, pair, min_hits, max_hits, **kw):
        lower, upper = self.window
        a, b = (self.data, None) if form == "interleaved" else (self.r1, self.r2)
        return ref.filter_fastq(a, self.k, self.items, b, lower=lower, upper=upper, min_hits=min_hits, max_hits=max_hits, pair=pair,
                                counts_cache=self.cache, **kw)


@functools.lru_cache(maxsize=None)
def _built(case):
    return _Built(case)


def _run(b, tmp_path, form, pair, min_hits, max_hits, tag="x", data=None, **kw):
    """(kept bytes 1, kept bytes 2 or None, the returned dict) of ``filter_fastq`` on files written for the call"""
    lower, upper = b.window
    if form == "interleaved":
        src = tmp_path / f"{tag}.fq"
        src.write_bytes(b.data if data is None else data)
        out = tmp_path / f"{tag}.out.fq"
        res = b.table.filter_fastq(str(src), str(out), lower=lower, upper=upper, min_hits=min_hits, max_hits=max_hits, pair=pair, **kw)
        return out.read_bytes(), None, res
    s1, s2, o1, o2 = (tmp_path / f"{tag}.{n}.fq" for n in ("r1", "r2", "o1", "o2"))
    s1.write_bytes(b.r1 if data is None else data[0])
    s2.write_bytes(b.r2 if data is None else data[1])
    res = b.table.filter_fastq(str(s1), str(o1), str(s2), str(o2), lower=lower, upper=upper, min_hits=min_hits, max_hits=max_hits, pair=pair, **kw)
    return o1.read_bytes(), o2.read_bytes(), res


def _same(got, want):
    g1, g2, res = got
    w1, w2, tot = want
    assert g1 == w1 and g2 == w2
    assert {n: res[n] for n in tot} == tot
    assert set(res) == set(tot) | {"seconds", "device_ms"} and res["seconds"] > 0 and res["device_ms"] >= 0
    for n in tot:
        assert type(res[n]) is int


# ------------------------------------------------------------------------------------------------------------ 1. read_hits

@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_read_hits_of_every_record(case):
    b = _built(case)
    text = torch.frombuffer(bytearray(b.data), dtype=torch.uint8).to(DEV)
    n_records = len(b.records)
    assert 340 <= n_records <= 380
    seen = set()
    for lenient in (True, False):
        for mq in (None, "?"):
            for lower, upper in WINDOWS:
                got = b.table.read_hits(text, lower=lower, upper=upper, lowercase_is_base=lenient, min_qual_char=mq)
                assert got.dtype == torch.int64 and got.device == text.device and got.shape == (n_records, 2)
                want = ref.read_hits(b.data, b.k, b.items, lower, upper, lenient, mq, counts_cache=b.cache)
                bad = np.nonzero((got.cpu().numpy() != want).any(1))[0]
                assert len(bad) == 0, (lenient, mq, lower, upper, bad[:5], got[bad[:5]], want[bad[:5]])
                seen.add(want.tobytes())
    assert len(seen) >= 8                            # (the windows and rules ask different questions of this corpus)
    # a view that does not begin at a 16-byte boundary of its buffer, and nothing at all
    off = torch.cat([torch.zeros(3, dtype=torch.uint8, device=DEV), text])[3:]
    assert torch.equal(b.table.read_hits(off), b.table.read_hits(text))
    assert b.table.read_hits(text[:0]).shape == (0, 2)
    assert b.unchanged()


def test_read_hits_refuses_a_cpu_tensor_and_malformed_text():
    b = _built(CASES[1])
    good = b.records[0] + b.records[1]
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        b.table.read_hits(torch.frombuffer(bytearray(good), dtype=torch.uint8))

    def dev(data):
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)

    assert b.table.read_hits(dev(good)).shape == (2, 2)
    for data, record in ((good[:-5].rsplit(b"\n", 1)[0], 1), (good + b"\n", 2), (b"\n", 0), (good.replace(b"@", b"", 1), 0),
                         (b.records[0] + b.records[1].replace(b"\n+", b"\n-", 1) + b.records[2], 1)):
        with pytest.raises(ValueError, match=f"record {record}:"):
            b.table.read_hits(dev(data))
    short = b.records[0] + _record(b"short quality", b"ACGT" * 10, b"I" * 39)
    assert b.table.read_hits(dev(short)).shape == (2, 2)
    with pytest.raises(ValueError, match="record 1: its quality line is shorter"):
        b.table.read_hits(dev(short), min_qual_char="?")
    with pytest.raises(ValueError, match="upper"):
        b.table.read_hits(dev(good), lower=3, upper=2)
    assert b.unchanged()


# ------------------------------------------------------------------------------------------------------------ 2. filter_fastq

@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_filter_fastq_equals_the_reference(case, tmp_path):
    b = _built(case)
    fractions = []
    for form, pair in FORMS:
        for min_hits, max_hits in combos_of(b.k):
            want = b.want(form, pair, min_hits, max_hits)
            share = want[2]["kept"] / want[2]["records"]
            print(f"{_IDS[CASES.index(case)]} {form} {pair} min_hits={min_hits} max_hits={max_hits}: the reference keeps {share:.3f}")
            assert 0.1 <= share <= 0.9, (form, pair, min_hits, max_hits, share)
            _same(_run(b, tmp_path, form, pair, min_hits, max_hits), want)
            fractions.append(share)
    assert b.unchanged()
    assert sorted(os.listdir(tmp_path)) == sorted(n for n in os.listdir(tmp_path) if not n.endswith(".tmp"))


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[5]], ids=[_IDS[1], _IDS[4], _IDS[5]])
def test_quality_threshold_and_strict_case(case, tmp_path):
    b = _built(case)
    for kw in (dict(min_qual_char="?"), dict(lowercase_is_base=False), dict(min_qual_char="J", lowercase_is_base=False)):
        for form, pair in (("interleaved", "single"), ("r1r2", "any")):
            if kw.get("min_qual_char") == "J":       # no base is left: no read passes, whatever the bounds
                got = _run(b, tmp_path, form, pair, 0.0, None, **kw)
                assert got[0] == b"" and got[2]["kept"] == 0 and got[2]["kmers"] == 0 and got[2]["records"] == len(b.records)
                continue
            want = b.want(form, pair, 0.5, None, **kw)
            assert 0.1 <= want[2]["kept"] / want[2]["records"] <= 0.9
            _same(_run(b, tmp_path, form, pair, 0.5, None, **kw), want)
    assert b.want("interleaved", "single", 0.5, None, min_qual_char="?")[2] != b.want("interleaved", "single", 0.5, None)[2]
    assert b.unchanged()


@pytest.mark.parametrize("piece", [700, 4096])
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5]], ids=[_IDS[0], _IDS[3], _IDS[5]])
def test_pieces_give_the_one_piece_answer(case, piece, tmp_path, monkeypatch):
    b = _built(case)
    assert max(len(r) for r in b.records) > 2 * 4096 and min(len(r) for r in b.records) < 64     # a record beyond a piece; many to a piece
    whole = {f: _run(b, tmp_path, f, "any", 0.5, None, tag="whole") for f in ("interleaved", "r1r2")}
    monkeypatch.setenv("PG_FILTER_PIECE_BYTES", str(piece))
    for form in ("interleaved", "r1r2"):
        got = _run(b, tmp_path, form, "any", 0.5, None, tag="pieces")
        assert got[:2] == whole[form][:2]
        assert {n: v for n, v in got[2].items() if n not in ("seconds", "device_ms")} == {n: v for n, v in whole[form][2].items() if n not in ("seconds", "device_ms")}
        _same(got, b.want(form, "any", 0.5, None))
    assert b.unchanged()


@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=[_IDS[1], _IDS[3]])
def test_crlf_no_final_newline_and_gzip_select_the_same(case, tmp_path):
    b = _built(case)
    want = b.want("interleaved", "any", 0.5, None)
    keep = ref.passes(ref.read_hits(b.data, b.k, b.items, *b.window, counts_cache=b.cache), 0.5, None)
    keep = np.repeat(keep.reshape(-1, 2).any(1), 2)
    # CRLF: '\r' is a byte of its line and no base; the records leave as they came
    crlf = [r.replace(b"\n", b"\r\n") for r in b.records]
    got = _run(b, tmp_path, "interleaved", "any", 0.5, None, tag="crlf", data=b"".join(crlf))
    assert got[0] == b"".join(r for r, kp in zip(crlf, keep) if kp) and got[2]["kept"] == want[2]["kept"] and got[2]["kmers"] == want[2]["kmers"]
    _same(got, ref.filter_fastq(b"".join(crlf), b.k, b.items, lower=b.window[0], upper=b.window[1], min_hits=0.5, pair="any"))
    # no final newline: the last record (kept or not) is copied without one
    i = int(np.nonzero(keep)[0][0])                  # (the first record of a pair that stays)
    for recs in (b.records, b.records + [b.records[i], b.records[i + 1]]):
        data = b"".join(recs)[:-1]
        w = ref.filter_fastq(data, b.k, b.items, lower=b.window[0], upper=b.window[1], min_hits=0.5, pair="any")
        got = _run(b, tmp_path, "interleaved", "any", 0.5, None, tag="nonl", data=data)
        _same(got, w)
    assert got[0][-1:] != b"\n" and got[0].endswith(b.records[i] + b.records[i + 1][:-1])
    # gzip input, one file and two
    src = tmp_path / "reads.fq.gz"
    src.write_bytes(gzip.compress(b.data))
    out = tmp_path / "from_gz.fq"
    res = b.table.filter_fastq(str(src), str(out), lower=b.window[0], upper=b.window[1], min_hits=0.5, pair="any")
    _same((out.read_bytes(), None, res), want)
    s1, s2, o1, o2 = (tmp_path / n for n in ("r1.fq.gz", "r2.fq", "o1.fq", "o2.fq"))
    s1.write_bytes(gzip.compress(b.r1))
    s2.write_bytes(b.r2)
    res = b.table.filter_fastq(str(s1), str(o1), str(s2), str(o2), lower=b.window[0], upper=b.window[1], min_hits=0.5, pair="both")
    _same((o1.read_bytes(), o2.read_bytes(), res), b.want("r1r2", "both", 0.5, None))
    assert b.unchanged()


@pytest.mark.parametrize("piece", [None, 700])
def test_errors_name_the_record_and_leave_no_output(piece, tmp_path, monkeypatch):
    b = _built(CASES[4])
    if piece:
        monkeypatch.setenv("PG_FILTER_PIECE_BYTES", str(piece))
    recs = b.records
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
            b.table.filter_fastq(str(src), str(out), **kw)
        assert sorted(os.listdir(tmp_path)) == ["in.fq"]

    refused(cut, f"record {r}: the file ends inside it")
    refused(no_at, f"record {r}: its first line does not begin with '@'")
    refused(no_plus, f"record {r}: its third line does not begin with '\\+'")
    refused(short_q, f"record {r}: its quality line is shorter", min_qual_char="?")
    refused(odd, f"record {r - 1} has no mate", pair="any")
    refused(odd, f"record {r - 1} has no mate", pair="both")
    src = tmp_path / "in.fq"
    src.write_bytes(short_q)                         # without the threshold the quality line is never looked at, and an odd count is fine
    assert b.table.filter_fastq(str(src), str(out), pair="any")["records"] == len(recs)
    src.write_bytes(odd)
    assert b.table.filter_fastq(str(src), str(out), pair="single")["records"] == r
    os.remove(out)
    os.remove(src)
    # R1 / R2 of different length, either way round
    s1, s2, o1, o2 = (tmp_path / n for n in ("r1.fq", "r2.fq", "o1.fq", "o2.fq"))
    for a, c in ((b.r1, b"".join(recs[1::2][:-3])), (b"".join(recs[0::2][:-3]), b.r2)):
        s1.write_bytes(a)
        s2.write_bytes(c)
        with pytest.raises(ValueError, match="same number of records"):
            b.table.filter_fastq(str(s1), str(o1), str(s2), str(o2))
        assert sorted(os.listdir(tmp_path)) == ["r1.fq", "r2.fq"]
    # an output that asks for gzip, and arguments that make no sense: refused before anything is opened
    s1.write_bytes(b.data)
    for kw, match in ((dict(out1=str(tmp_path / "o.fq.gz")), "plain text"), (dict(out1=str(o1), pair="all"), "pair must be"),
                      (dict(out1=str(o1), min_hits=1.5), "share"), (dict(out1=str(o1), min_hits=-1), "at least 0"),
                      (dict(out1=str(o1), src2=str(s2)), "go together"),
                      (dict(out1=str(s1)), "must differ"), (dict(out1=str(o1), src2=str(s2), out2=str(o1)), "must differ"),
                      (dict(out1=str(o1), src2=str(s2), out2=str(s1)), "must differ"), (dict(out1=str(o1), src2=str(s2), out2=str(o2), pair="single"), "ONE file"),
                      (dict(out1=str(o1), lower=3, upper=2), "upper"), (dict(out1=str(o1), min_qual_char="??"), "one character")):
        with pytest.raises(ValueError, match=match):
            b.table.filter_fastq(str(s1), **kw)
        assert sorted(os.listdir(tmp_path)) == ["r1.fq", "r2.fq"]
    with pytest.raises(OSError):
        b.table.filter_fastq(str(tmp_path / "not_there.fq"), str(o1))
    assert sorted(os.listdir(tmp_path)) == ["r1.fq", "r2.fq"]
    assert b.unchanged()


# ------------------------------------------------------------------------------------------------------------ 3. the tool

def _main(argv):
    try:
        return cli.main_kmer_table(argv)
    except SystemExit as e:
        return e.code


def test_kmer_table_filter_from_a_dump_and_from_the_reads_themselves(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    b = _built(CASES[3])
    k = b.k
    (tmp_path / "reads.fq").write_bytes(b.data)
    (tmp_path / "r1.fq").write_bytes(b.r1)
    (tmp_path / "r2.fq").write_bytes(b.r2)
    b.table.write_dump("table.dump")
    capsys.readouterr()
    # -g: the table of the dump; R1 / R2, a share, both mates must pass
    assert _main(["filter", "-g", "table.dump", "-k", str(k), "-1", "r1.fq", "-2", "r2.fq", "-o", "o1.fq", "-o2", "o2.fq", "--min-hits", "0.5",
                  "--pair", "both"]) == 0
    out = capsys.readouterr()
    lines = out.out.splitlines()
    assert len(lines) == 1 and out.err == ""
    _same(((tmp_path / "o1.fq").read_bytes(), (tmp_path / "o2.fq").read_bytes(), json.loads(lines[0])), b.want("r1r2", "both", 0.5, None))
    # no table source: the table is counted from the reads themselves; k-mers seen once are the errors' (and the foreign reads')
    from oracle import oracle
    seqs = b"".join(s.upper() + b"N" for _, _, s, _ in ref.records_of(b.data))      # (the tables count lower-case bases)
    codes, counts = oracle.Table(k, threads=4).count(seqs).items()
    own = (codes, counts.astype(np.int64))
    want = ref.filter_fastq(b.data, k, own, lower=2, min_hits=3, pair="single")
    assert 0.1 <= want[2]["kept"] / want[2]["records"] <= 0.9
    assert _main(["filter", "-k", str(k), "-i", "reads.fq", "-o", "solid.fq", "-L", "2", "--min-hits", "3", "--pair", "single"]) == 0
    out = capsys.readouterr()
    assert len(out.out.splitlines()) == 1 and out.err == ""
    _same(((tmp_path / "solid.fq").read_bytes(), None, json.loads(out.out)), want)
    # exit 1 and a message: a missing input, a share above 1, mates asked of a file that has none
    (tmp_path / "odd.fq").write_bytes(b"".join(b.records[:3]))
    before = sorted(os.listdir(tmp_path))
    for argv, text in ((["filter", "-g", "table.dump", "-k", str(k), "-i", "not_there.fq", "-o", "x.fq"], "not_there.fq"),
                       (["filter", "-g", "table.dump", "-k", str(k), "-i", "reads.fq", "-o", "x.fq", "--min-hits", "1.5"], "--min-hits"),
                       (["filter", "-g", "table.dump", "-k", str(k), "-i", "odd.fq", "-o", "x.fq", "--pair", "both"], "has no mate")):
        assert _main(argv) == 1
        out = capsys.readouterr()
        assert out.out == "" and out.err.startswith("kmer_table: ") and text in out.err
        assert sorted(os.listdir(tmp_path)) == before
    assert b.unchanged()
