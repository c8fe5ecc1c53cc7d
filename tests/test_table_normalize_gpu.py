"""Read depth normalised from a finished k-mer table: ``KmerTable.read_depths`` / ``KmerTable.normalize_fastq`` (pg_fastq_index,
pg_table_read_depths, pg_fastq_gather) and ``kmer_table normalize`` -- what BBNorm and khmer's normalize-by-median do, beside the
read set of scripts/low_abd_reads.sh:10 (extract_unmapped.cpp).

Everything is integers and bytes, compared exactly with tests/_normalize_ref.py (a plain restatement of the semantics in
include/pangaea_feat.h).  One table per kind at the filter tests' geometries, each counted from the corpus's own reads; one
corpus and one set of reference counts per table, shared by the tests; every table is cloned when it is built and compared with
its clone after each test.

THE CORPUS.  A community of two: genome H (3 000 bases, 400 pairs: about 40 x) and genome L (30 000 bases, 400 pairs: about
4 x), fragments of 400 bases, reads of 150 with 1 % substitutions; 100 pairs of a genome nobody else saw; 40 pairs of one H mate
and one foreign mate; shuffled.  For the table of one 2^14-slot bucket it is scaled down (H 600 bases and 50 pairs, L 4 000 and
50, 12 foreign and 6 mixed pairs).  The table is counted from these reads.  Behind them the edge records, which the table has
not seen: sequence lines of 0, 1, k - 1, k, k + 1 bases, of 63 .. 65, 511 .. 513, 1 500 and 5 000 positions spliced from H, L and
foreign text (so that their order statistics are not trivial, in the registers and in every digit sweep of the long form), N at
either end and in the middle, all N, lower case, CRLF, a quality line longer than its sequence.

THE BAND.  Every ``normalize_fastq`` case is asserted, on the reference's own result, to keep between 10 % and 90 % of the
records: (target, min_depth) in {(8, 0), (8, 2), (20, 2), (3, 0)} for every form and seed.  The dense k = 4 table's depths are in
the thousands whatever the read: there the target is half the reference's median record depth and min_depth 0."""
import functools
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pangaea_amd import kmer
from pangaea_amd.reads import ReadStream

from . import _normalize_ref as ref
from .conftest import ROOT
from .test_table_filter_gpu import CASES, DEV, FORMS, _IDS, _alloc, _record

pytestmark = pytest.mark.gpu

COMBOS = [(8, 0), (8, 2), (20, 2), (3, 0)]
SEEDS = [0, 2023]
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def corpus_of(k: int, small: bool, seed: int) -> tuple:
    """(the records the table is counted from, mates next to each other; the edge records)"""
    rng = np.random.RandomState(seed)

    def rand(n):
        return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))

    H, L, F = rand(600 if small else 3000), rand(4000 if small else 30_000), rand(200_000)
    n_h, n_l, n_f, n_mixed = (50, 50, 12, 6) if small else (400, 400, 100, 40)

    def mates(genome):
        at = int(rng.randint(len(genome) - 400 + 1))
        frag = genome[at:at + 400]
        out = []
        for read in (frag[:150], frag[-150:].translate(_RC)[::-1]):
            seq = bytearray(read)
            for p in np.nonzero(rng.rand(150) < 0.01)[0]:
                seq[p] = rng.choice([c for c in b"ACGT" if c != seq[p]])
            out.append(bytes(seq))
        return out

    def quality(n):
        q = np.full(n, ord("I"), np.uint8)
        if rng.rand() < 0.3:
            q[rng.rand(n) < 0.1] = ord("#")
        return bytes(q)

    pairs = [mates(H) for _ in range(n_h)] + [mates(L) for _ in range(n_l)] + [mates(F) for _ in range(n_f)]
    for i in range(n_mixed):
        a, b = mates(H)[0], mates(F)[1]
        pairs.append([a, b] if i % 2 else [b, a])
    recs = []
    for i in rng.permutation(len(pairs)):
        for m, seq in enumerate(pairs[i]):
            name = b"p%d/%d" % (i, m + 1) if i % 3 else b"p%d\tBX:Z:ACGTACGTACGTACGT-1" % i
            recs.append(_record(name, seq, quality(len(seq)), b"+" + name if i % 5 == 0 else b"+"))

    def spliced(n):
        """n bases: pieces of H, L and foreign text (two, two and one in five), 60 to 200 bases each"""
        out = b""
        while len(out) < n:
            g = (H, H, L, L, F)[int(rng.randint(5))]
            m = int(rng.randint(60, 200))
            at = int(rng.randint(len(g) - m))
            out += g[at:at + m]
        return out[:n]

    edges = [b"", b"A", spliced(k - 1), spliced(k), spliced(k + 1)]
    edges += [spliced(n_pos + k - 1) for n_pos in (63, 64, 65, 511, 512, 513, 1500, 5000)]
    r = mates(H)[0]
    edges += [b"N" + r[1:], r[:-1] + b"N", r[:75] + b"N" + r[76:], b"N" * 150, r.lower(), mates(L)[1].lower()]
    tail = [_record(b"edge%d len=%d" % (i, len(seq)), seq) for i, seq in enumerate(edges)]
    tail.append(_record(b"crlf", mates(H)[1]).replace(b"\n", b"\r\n"))
    tail.append(_record(b"crlf long", spliced(700)).replace(b"\n", b"\r\n"))
    tail.append(_record(b"long quality", r[:100], b"I" * 120))
    if len(tail) % 2:
        tail.append(_record(b"the last one's mate", mates(L)[0]))
    return recs, tail


class _Built:
    def __init__(self, case):
        kind, k, log2_slots, log2_bucket = case
        self.k, self.kind = k, kind
        counted, edges = corpus_of(k, log2_slots == 14, 1200 + k)
        self.records = counted + edges
        stream = ReadStream.from_runs([("corpus", b"".join(r.split(b"\n")[1] + b"N" for r in counted))], device=DEV)
        self.table = _alloc(kind, k, log2_slots, log2_bucket).count(stream)
        assert self.table.kind == kind
        self.clone = self.table.data.clone()
        codes, counts = self.table.items()
        self.items = (codes, counts.astype(np.int64))
        self.data = b"".join(self.records)
        self.r1, self.r2 = b"".join(self.records[0::2]), b"".join(self.records[1::2])
        self.cache = {}

    def unchanged(self):
        return torch.equal(self.table.data, self.clone)

    def combos(self):
        if self.k != 4:
            return COMBOS
        d = ref.read_depths(self.data, self.k, self.items, cache=self.cache)[:, 2]
        return [(max(1, int(np.median(d)) // 2), 0)]

    def want(self, form, pair, target, min_depth, **kw):
        a, b = (self.data, None) if form == "interleaved" else (self.r1, self.r2)
        return ref.normalize_fastq(a, self.k, self.items, b, target=target, min_depth=min_depth, pair=pair, cache=self.cache, **kw)


@functools.lru_cache(maxsize=None)
def _built(case):
    return _Built(case)


def _dev(data: bytes) -> torch.Tensor:
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)


def _run(b, tmp_path, form, pair, target, min_depth, tag="x", data=None, table=None, **kw):
    """(kept bytes 1, kept bytes 2 or None, the returned dict) of ``normalize_fastq`` on files written for the call"""
    table = b.table if table is None else table
    if form == "interleaved":
        src = tmp_path / f"{tag}.fq"
        src.write_bytes(b.data if data is None else data)
        out = tmp_path / f"{tag}.out.fq"
        res = table.normalize_fastq(str(src), str(out), target=target, min_depth=min_depth, pair=pair, **kw)
        return out.read_bytes(), None, res
    s1, s2, o1, o2 = (tmp_path / f"{tag}.{n}.fq" for n in ("r1", "r2", "o1", "o2"))
    s1.write_bytes(b.r1 if data is None else data[0])
    s2.write_bytes(b.r2 if data is None else data[1])
    res = table.normalize_fastq(str(s1), str(o1), str(s2), str(o2), target=target, min_depth=min_depth, pair=pair, **kw)
    return o1.read_bytes(), o2.read_bytes(), res


def _same(got, want):
    g1, g2, res = got
    w1, w2, tot = want
    assert g1 == w1 and g2 == w2
    assert {n: res[n] for n in tot} == tot
    assert set(res) == set(tot) | {"seconds", "device_ms"} and res["seconds"] > 0 and res["device_ms"] >= 0
    for n in tot:
        assert type(res[n]) is int


def _totals(res):
    return {n: v for n, v in res.items() if n not in ("seconds", "device_ms")}


# ------------------------------------------------------------------------------------------------------------ 1. read_depths

def _rows_equal(table, k, items, data, text, cache, **kw):
    got = table.read_depths(text, **kw)
    want = ref.read_depths(data, k, items, cache=cache, **kw)
    assert got.dtype == torch.int64 and got.device == text.device and got.shape == want.shape
    bad = np.nonzero((got.cpu().numpy() != want).any(1))[0]
    assert len(bad) == 0, (kw, bad[:5], got[bad[:5]], want[bad[:5]])
    return want


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_read_depths_of_every_record(case):
    b = _built(case)
    text = _dev(b.data)
    seen = set()
    for lenient in (True, False):
        for mq in (None, "?"):
            for lower in (1, 3):
                for percentile in (0, 25, 50, 54, 100):
                    want = _rows_equal(b.table, b.k, b.items, b.data, text, b.cache, lower=lower, percentile=percentile, lowercase_is_base=lenient,
                                       min_qual_char=mq)
                    seen.add(want.tobytes())
    assert len(seen) >= (8 if b.k == 4 else 20)      # (the percentiles, bounds and rules ask different questions of this corpus)
    # the forms the kernel takes are all in the corpus, none with a trivial answer: records that fill the registers to the
    # last lane and one more, and long ones whose order statistics differ
    rows = {p: ref.read_depths(b.data, b.k, b.items, percentile=p, cache=b.cache) for p in (0, 50, 100)}
    n = rows[50][:, 0]
    assert {63, 64, 65, 511, 512, 513, 1500, 5000} <= set(n.tolist())
    for size in (512, 513, 1500, 5000):
        r = int(np.nonzero(n == size)[0][0])
        d0, d50, d100 = (int(rows[p][r, 2]) for p in (0, 50, 100))
        assert d0 < d100 and (size < 5000 or d0 < d50 < d100), (size, d0, d50, d100)
    # a view that does not begin at a 16-byte boundary of its buffer, and nothing at all
    off = torch.cat([torch.zeros(3, dtype=torch.uint8, device=DEV), text])[3:]
    assert torch.equal(b.table.read_depths(off), b.table.read_depths(text))
    assert b.table.read_depths(text[:0]).shape == (0, 3)
    assert b.unchanged()


def test_read_depths_past_2_to_the_21():
    """a wide k = 31 table of the corpus's counts x 70 001: every digit of the long form and the high bits of the short one carry
    information"""
    b = _built(CASES[2])
    codes, counts = b.items
    items = (codes, counts * 70_001)
    table = kmer.KmerTable.from_items(b.k, codes, items[1], DEV, kind="wide")
    clone = table.data.clone()
    assert table.kind == "wide" and items[1].max() > 1 << 21
    text, cache = _dev(b.data), {}
    top = 0
    for lower, percentile in ((1, 0), (1, 50), (1, 54), (1, 100), (70_002, 50), (70_002, 25), (3 * 70_001, 100)):
        want = _rows_equal(table, b.k, items, b.data, text, cache, lower=lower, percentile=percentile)
        top = max(top, int(want[want[:, 0] > 512, 2].max()))
    assert top > 1 << 21                             # (a long record's answer has a digit in the third byte)
    assert torch.equal(table.data, clone) and b.unchanged()


def test_read_depths_refuses_a_cpu_tensor_and_malformed_text():
    b = _built(CASES[1])
    good = b.records[0] + b.records[1]
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        b.table.read_depths(torch.frombuffer(bytearray(good), dtype=torch.uint8))
    with pytest.raises(TypeError):
        b.table.read_depths(good)
    assert b.table.read_depths(_dev(good)).shape == (2, 3)
    for data, record in ((good[:-5].rsplit(b"\n", 1)[0], 1), (good + b"\n", 2), (b"\n", 0), (good.replace(b"@", b"", 1), 0),
                         (b.records[0] + b.records[1].replace(b"\n+", b"\n-", 1) + b.records[2], 1)):
        with pytest.raises(ValueError, match=f"record {record}:"):
            b.table.read_depths(_dev(data))
    short = b.records[0] + _record(b"short quality", b"ACGT" * 10, b"I" * 39)
    assert b.table.read_depths(_dev(short)).shape == (2, 3)
    with pytest.raises(ValueError, match="record 1: its quality line is shorter"):
        b.table.read_depths(_dev(short), min_qual_char="?")
    for kw, match in ((dict(lower=0), "lower"), (dict(percentile=101), "percentile"), (dict(percentile=-1), "percentile"),
                      (dict(percentile=50.0), "percentile"), (dict(min_qual_char="??"), "one character")):
        with pytest.raises(ValueError, match=match):
            b.table.read_depths(_dev(good), **kw)
    assert b.unchanged()


# ------------------------------------------------------------------------------------------------------------ 2. normalize_fastq

# (the dense k = 4 table has one case, its target from the reference: the module's docstring)
_MATRIX = [(c, i) for c in CASES for i in range(1 if c[1] == 4 else len(COMBOS))]


@pytest.mark.parametrize("case,combo", _MATRIX, ids=[f"{_IDS[CASES.index(c)]}-" + ("half-median" if c[1] == 4 else "t%d-m%d" % COMBOS[i]) for c, i in _MATRIX])
def test_normalize_fastq_equals_the_reference(case, combo, tmp_path):
    b = _built(case)
    target, min_depth = b.combos()[combo]
    for form, pair in FORMS:
        kept = []
        for seed in SEEDS:
            want = b.want(form, pair, target, min_depth, seed=seed)
            share = want[2]["kept"] / want[2]["records"]
            print(f"{_IDS[CASES.index(case)]} {form} {pair} target={target} min_depth={min_depth} seed={seed}: the reference keeps {share:.3f}")
            assert 0.1 <= share <= 0.9, (form, pair, target, min_depth, seed, share)
            _same(_run(b, tmp_path, form, pair, target, min_depth, seed=seed), want)
            kept.append(want[0])
        assert kept[0] != kept[1]                    # (another seed, another choice)
    assert b.unchanged()
    assert sorted(os.listdir(tmp_path)) == sorted(n for n in os.listdir(tmp_path) if not n.endswith(".tmp"))


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[5]], ids=[_IDS[1], _IDS[4], _IDS[5]])
def test_lower_percentile_quality_threshold_and_strict_case(case, tmp_path):
    b = _built(case)
    plain = b.want("interleaved", "single", 8, 2)[2]
    for kw in (dict(min_qual_char="?"), dict(lowercase_is_base=False), dict(lower=3, percentile=25), dict(percentile=100),
               dict(min_qual_char="J", lowercase_is_base=False)):
        for form, pair in (("interleaved", "single"), ("r1r2", "any")):
            if kw.get("min_qual_char") == "J":       # no base is left: no k-mer, nothing is kept, every record is low
                got = _run(b, tmp_path, form, pair, 8, 0, **kw)
                n = len(b.records)
                assert got[0] == b"" and got[2]["kept"] == 0 and got[2]["kmers"] == 0 and got[2]["records"] == n and got[2]["low"] == n
                continue
            want = b.want(form, pair, 8, 2, **kw)
            assert 0.1 <= want[2]["kept"] / want[2]["records"] <= 0.9
            _same(_run(b, tmp_path, form, pair, 8, 2, **kw), want)
        if kw.get("min_qual_char") != "J":
            assert b.want("interleaved", "single", 8, 2, **kw)[2] != plain
    assert b.unchanged()


@pytest.mark.parametrize("piece", [700, 4096])
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5]], ids=[_IDS[0], _IDS[3], _IDS[5]])
def test_pieces_give_the_one_piece_answer(case, piece, tmp_path, monkeypatch):
    b = _built(case)
    assert max(len(r) for r in b.records) > 2 * 4096 and min(len(r) for r in b.records) < 64     # a record beyond a piece; many to a piece
    target, min_depth = b.combos()[0]
    forms = (("interleaved", "any"), ("interleaved", "single"), ("r1r2", "both"))
    whole = {f: _run(b, tmp_path, *f, target, min_depth, tag="whole", seed=5) for f in forms}
    monkeypatch.setenv("PG_FILTER_PIECE_BYTES", str(piece))
    for f in forms:
        got = _run(b, tmp_path, *f, target, min_depth, tag="pieces", seed=5)
        assert got[:2] == whole[f][:2] and _totals(got[2]) == _totals(whole[f][2])
        _same(got, b.want(*f, target, min_depth, seed=5))
    assert b.unchanged()


def test_gzip_input_equals_plain_input(tmp_path):
    b = _built(CASES[1])
    src = tmp_path / "reads.fq.gz"
    src.write_bytes(gzip.compress(b.data))
    out = tmp_path / "from_gz.fq"
    res = b.table.normalize_fastq(str(src), str(out), target=8, min_depth=2, seed=9)
    _same((out.read_bytes(), None, res), b.want("interleaved", "any", 8, 2, seed=9))
    s1, s2, o1, o2 = (tmp_path / n for n in ("r1.fq.gz", "r2.fq", "o1.fq", "o2.fq"))
    s1.write_bytes(gzip.compress(b.r1))
    s2.write_bytes(b.r2)
    res = b.table.normalize_fastq(str(s1), str(o1), str(s2), str(o2), target=8, min_depth=2, pair="both", seed=9)
    _same((o1.read_bytes(), o2.read_bytes(), res), b.want("r1r2", "both", 8, 2, seed=9))
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
            b.table.normalize_fastq(str(src), str(out), target=8, **kw)
        assert sorted(os.listdir(tmp_path)) == ["in.fq"]

    refused(cut, f"record {r}: the file ends inside it")
    refused(no_at, f"record {r}: its first line does not begin with '@'")
    refused(no_plus, f"record {r}: its third line does not begin with '\\+'")
    refused(short_q, f"record {r}: its quality line is shorter", min_qual_char="?")
    refused(odd, f"record {r - 1} has no mate", pair="any")
    refused(odd, f"record {r - 1} has no mate", pair="both")
    src = tmp_path / "in.fq"
    src.write_bytes(odd)
    assert b.table.normalize_fastq(str(src), str(out), target=8, pair="single")["records"] == r
    os.remove(out)
    # arguments that make no sense: refused before anything is opened
    for kw, match in ((dict(), "target"), (dict(target=0), "target"), (dict(target=1 << 31), "target"), (dict(target=8.0), "target"),
                      (dict(target=8, min_depth=-1), "min_depth"), (dict(target=8, seed=-1), "seed"), (dict(target=8, seed=1 << 64), "seed"),
                      (dict(target=8, lower=0), "lower"), (dict(target=8, percentile=101), "percentile"), (dict(target=8, pair="all"), "pair must be"),
                      (dict(target=8, min_qual_char="??"), "one character")):
        with pytest.raises(ValueError, match=match):
            b.table.normalize_fastq(str(src), str(out), **kw)
        assert sorted(os.listdir(tmp_path)) == ["in.fq"]
    with pytest.raises(ValueError, match="plain text"):
        b.table.normalize_fastq(str(src), str(tmp_path / "o.fq.gz"), target=8)
    assert sorted(os.listdir(tmp_path)) == ["in.fq"]
    assert b.unchanged()


# ------------------------------------------------------------------------------------------------------------ 3. the tool

def test_kmer_table_normalize_with_the_reads_own_table(tmp_path):
    """one call of the tool in a process of its own, no table source: its file and its JSON line are those of
    ``count_kmers(...).normalize_fastq(...)`` on the same file"""
    b = _built(CASES[1])
    k = b.k
    src, out, mine = tmp_path / "reads.fq", tmp_path / "tool.fq", tmp_path / "mine.fq"
    src.write_bytes(b.data)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    tool = subprocess.run([sys.executable, os.path.join(ROOT, "pangaea_amd", "bin", "kmer_table"), "normalize", "-k", str(k), "-i", str(src),
                           "--target", "8", "--min-depth", "2", "--seed", "77", "--pair", "both", "-o", str(out)],
                          capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert tool.returncode == 0, tool.stderr               # (stderr is the driver's to write to as well)
    lines = tool.stdout.splitlines()
    assert len(lines) == 1
    table = kmer.count_kmers(ReadStream.from_fastq(str(src), None, device=DEV).to(DEV), k, lowercase_is_base=True)    # (the tool's rule)
    res = table.normalize_fastq(str(src), str(mine), target=8, min_depth=2, seed=77, pair="both")
    assert out.read_bytes() == mine.read_bytes() and _totals(json.loads(lines[0])) == _totals(res)
    assert 0.1 <= res["kept"] / res["records"] <= 0.9 and res["records"] == len(b.records)
    assert b.unchanged()
