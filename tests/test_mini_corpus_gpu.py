"""The super-k-mer kernels on the edge-case corpus of tests/_corpus.py, at every k from 13 to 31.

What ``synth.generate`` never gives the per-word segmentation (RowBits, mini_minimizers with its delay line, mini_record_ends with
the cap loop) and the kernels built on it: reads of every length from 0 to 2k + 40, an N and a soft-masked stretch at each of the
32 positions of a word, periodic reads that reach the record cap, palindromic M-mers and k-mers, every read's reverse complement,
every read a row of its own or cut into two rows inside a record, a k-mer across the 4096-word chunk boundary and one across a
512-word round boundary.

Integer results, compared bit for bit.  Expected values: ``oracle.Table(k).count(text)``, ``oracle.abd_row`` of every read's raw
text (``Laid.rows_by_oracle`` for the reads in two rows), ``oracle.tnf_row`` at k_tnf = 4 -- computed once per k (``_case``), on
a reference that tests/test_mini_corpus_host.py checks by itself.  (window, vsize) = (1, 64) drops the counts from 64 up, which the periodic reads exceed; (10, 400) drops nothing.
Three checks need no oracle: the reverse complemented stream, a shift against the word grid, a smaller record cap.  The fused
count goes through the checked build first."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import oracle
from pangaea_amd import kmer
from pangaea_amd.reads import ReadStream

from . import _corpus
from .conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = list(range(13, 32))
PACKED = [k for k in KS if k <= 21]              # packed mini tables: the pieces and the find form exist for these
EMITS = [(1, 64), (10, 400)]
GEOMETRY = {"first-pass": (18, 10),              # 2^8 buckets: the first scatter pass alone
            "both-passes": (20, 10)}             # 2^10 buckets of 2^10 slots: both passes (a wide table's bucket holds up to 2^13)
CASES = [pytest.param(k, g, id=f"k{k}-{g}") for k in KS for g in GEOMETRY]
ALL_SHIFTS = (13, 15, 16, 21, 22, 27, 31)        # every shift 1 .. 31 at these k, four shifts at the others
CAP_KS = (13, 16, 21, 25, 31)
UNWRITTEN = 0x7FFF_FFFF_FFFF                     # a fresh table is never cleared: every slot must be overwritten


def _ids(ks):
    return [pytest.param(k, id=f"k{k}") for k in ks]


def _abd_rows(laid, k, table, window, vsize):
    return laid.rows_by_oracle(lambda seq: oracle.abd_row(seq, k, table, window, vsize)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(k):
    """the corpus at this k and everything the oracle says about it; shared by the tests, never written to"""
    reads = _corpus.corpus(k)
    laid = _corpus.stream_of(reads, 0, k)
    table = oracle.Table(k, threads=4).count(laid.text)
    _corpus.check_against_oracle(laid, k, table)
    lenient = oracle.Table(k, threads=4).count(laid.text.upper())
    c = SimpleNamespace(k=k, reads=reads, laid=laid, table=table, items=table.items(), lenient_items=lenient.items(),
                        tnf=laid.rows_by_oracle(lambda seq: oracle.tnf_row(seq, 4)).astype(np.int32),
                        abd={e: _abd_rows(laid, k, table, *e) for e in EMITS},
                        abd_lenient={e: _abd_rows(laid, k, lenient, *e) for e in EMITS},
                        n_with_kmer=_corpus.n_reads_with_a_kmer(laid, k), records={})
    assert all(int(c.abd[e].sum()) > 0 for e in EMITS) and c.abd[(1, 64)].sum() < c.abd[(10, 400)].sum()
    assert not np.array_equal(c.abd[(10, 400)], c.abd_lenient[(10, 400)])
    return c


def _on_gpu(laid):
    s = ReadStream.from_runs(laid.runs, device=DEV)
    assert s.n_words >= laid.n_words > 4096 + 512 and s.valid_lower is not None       # (the stream pads to whole blocks of words)
    rows = laid.rows()
    plan = kmer.Plan(rows, DEV)
    assert plan.shuffle_ok
    return s, rows, plan


def _same_items(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _np(t):
    return t.cpu().numpy()


def _fused(k, geometry, s, plan, emit, **kw):
    t = kmer.KmerTable.mini_with_slots(k, DEV, *GEOMETRY[geometry])
    t.data.fill_(UNWRITTEN)
    t.count(s, rows=plan, emit=emit, **kw)
    assert t.kind == ("mini" if k <= 21 else "miniw") and t._emitted == emit
    assert t.n_buckets == (1 << 8 if geometry == "first-pass" else 1 << 10)
    return t


def _child(selection, n_tests, **env):
    """the selected tests of this file in a pytest process of their own, one at a time, under a time limit"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_mini_corpus_gpu.py"), "-k", selection],
                       cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"{n_tests} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ------------------------------------------------------------------ the checked build first


def test_fused_count_through_the_checked_build_first():
    """the same library built with -DPG_CHECKED (every global store of the super-k-mer kernels checks its index against the
    capacity of the buffer it writes into; PG_STATUS_BOUNDS instead of a memory fault): the fused count of this file runs
    through it in a process of its own, before anything here runs on the product.  See DESIGN.md section 4, 'the abort'."""
    if os.environ.get("PANGAEA_LIB") == "checked":
        pytest.skip("already inside the checked pass")
    _child("test_fused_count_and_lookups", len(CASES), PANGAEA_LIB="checked")


# ------------------------------------------------------------------ against the oracle


@pytest.mark.parametrize("k,geometry", CASES)
def test_fused_count_and_lookups(k, geometry, monkeypatch):
    """pg_mini_plan + pg_mini_count with the lookups inside, into a table full of garbage: the table, the rows from the emitted
    words, TNF; then the same rows by the find form (k <= 21) and by the lookup kernel on that table"""
    c = _case(k)
    s, rows, plan = _on_gpu(c.laid)
    for emit in EMITS:
        t = _fused(k, geometry, s, plan, emit)
        # the plan's record counts against a count in Python (tests/_corpus.py: count_records), under the cap in force
        forced = int(os.environ.get("PG_MINI_CAP") or 0)
        if forced not in c.records:
            c.records[forced] = _corpus.count_records(c.laid, k, forced or None)
        assert t._mini_pieces == 1 and (t._mini_plan.n_records, t._mini_plan.n_long) == c.records[forced]
        assert c.records[forced][0] > c.n_with_kmer                                     # (at least one record per read with a k-mer)
        assert _same_items(t.items(), c.items)
        tnf, abd = kmer.features(s, plan, k_tnf=4, table=t, window=emit[0], vsize=emit[1])
        assert t._emitted is None
        assert np.array_equal(_np(tnf), c.tnf) and np.array_equal(_np(abd), c.abd[emit])
        _, abd_f = kmer.features(s, rows, k_tnf=None, table=t, window=emit[0], vsize=emit[1], seg_chars=32)
        assert t.rows_form == ("find" if k <= 21 else None) and np.array_equal(_np(abd_f), c.abd[emit])
        monkeypatch.setenv("PG_MINI_FIND", "0")
        tnf_l, abd_l = kmer.features(s, rows, k_tnf=4, table=t, window=emit[0], vsize=emit[1], seg_chars=32)
        monkeypatch.delenv("PG_MINI_FIND")
        assert np.array_equal(_np(tnf_l), c.tnf) and np.array_equal(_np(abd_l), c.abd[emit])
        assert _same_items(t.items(), c.items)                                          # (the lookups only read)


@pytest.mark.parametrize("form", ["PG_MINI_MERGE=0", "PG_MINI_PROBE_TWICE=1"])
@pytest.mark.parametrize("k", _ids(KS))
def test_other_lookup_forms(k, form, monkeypatch):
    """the word-wise lookups and the general form (records probed a second time) inside the count"""
    monkeypatch.setenv(*form.split("="))
    c = _case(k)
    s, rows, plan = _on_gpu(c.laid)
    for emit in EMITS:
        t = _fused(k, "both-passes", s, plan, emit)
        assert _same_items(t.items(), c.items)
        _, abd = kmer.features(s, plan, k_tnf=None, table=t, window=emit[0], vsize=emit[1])
        assert np.array_equal(_np(abd), c.abd[emit])


@pytest.mark.parametrize("k", _ids(PACKED))
def test_counted_in_the_smallest_pieces(k, monkeypatch):
    """PANGAEA_MINI_PIECE_WORDS=256: some twenty pieces, reads across every seam -- the table and the rows of ONE count"""
    monkeypatch.delenv("PG_MINI_MERGE", raising=False)           # (the pieces keep the merged lookups)
    c = _case(k)
    s, rows, plan = _on_gpu(c.laid)
    for emit in EMITS:
        one = _fused(k, "both-passes", s, plan, emit)
        assert one._mini_pieces == 1
        want_items = one.items()
        _, want = kmer.features(s, plan, k_tnf=None, table=one, window=emit[0], vsize=emit[1])
        monkeypatch.setenv("PANGAEA_MINI_PIECE_WORDS", "256")
        t = _fused(k, "both-passes", s, plan, emit)
        monkeypatch.delenv("PANGAEA_MINI_PIECE_WORDS")
        assert t._mini_pieces == -(-s.n_words // 256) >= 16
        assert _same_items(t.items(), want_items) and _same_items(t.items(), c.items)
        _, abd = kmer.features(s, plan, k_tnf=None, table=t, window=emit[0], vsize=emit[1])
        assert torch.equal(abd, want) and np.array_equal(_np(abd), c.abd[emit])


@pytest.mark.parametrize("k", _ids(KS))
def test_lowercase_is_base(k):
    """the table under jellyfish's rule (soft-masked bases count), the rows under the reference's own (they do not)"""
    c = _case(k)
    s, rows, plan = _on_gpu(c.laid)
    for emit in EMITS:
        t = _fused(k, "both-passes", s, plan, emit, lowercase_is_base=True)
        assert _same_items(t.items(), c.lenient_items)
        _, abd = kmer.features(s, plan, k_tnf=None, table=t, window=emit[0], vsize=emit[1])
        assert np.array_equal(_np(abd), c.abd_lenient[emit])
        _, abd_l = kmer.features(s, rows, k_tnf=None, table=t, window=emit[0], vsize=emit[1], seg_chars=32)
        assert np.array_equal(_np(abd_l), c.abd_lenient[emit])


@pytest.mark.parametrize("find", ["PG_MINI_FIND=1", "PG_MINI_FIND=0"])
@pytest.mark.parametrize("holes", ["whole", "every-third-item-removed"])
@pytest.mark.parametrize("buckets", ["from_items", "256-buckets"])
@pytest.mark.parametrize("k", _ids(PACKED))
def test_abundance_of_a_finished_table(k, buckets, holes, find, monkeypatch):
    """``abundance_of`` (pg_mini_find, or the lookup kernel with PG_MINI_FIND=0) against a table made of the oracle's items --
    and of two thirds of them, so that k-mers the table lacks are looked up.  ``from_items`` sizes the table for its entries: a
    single bucket here, where the bucket of a record cannot be wrong; the same entries in 2^8 buckets are the other case."""
    monkeypatch.setenv(*find.split("="))
    c = _case(k)
    s, rows, plan = _on_gpu(c.laid)
    codes, counts = c.items
    if holes == "whole":
        otab, want = c.table, c.abd
    else:
        keep = np.arange(len(codes)) % 3 != 0
        codes, counts = codes[keep], counts[keep]
        otab = oracle.Table(k)
        for code, n in zip(codes.tolist(), counts.tolist()):
            otab.set(code, n)
        want = {e: _abd_rows(c.laid, k, otab, *e) for e in EMITS}
        assert all(0 < want[e].sum() < c.abd[e].sum() for e in EMITS)
    t = kmer.KmerTable.from_items(k, codes, counts, DEV, "mini")
    if buckets == "256-buckets":
        t = kmer.KmerTable.mini_with_slots(k, DEV, *GEOMETRY["first-pass"]).add_table(t)
    assert t.kind == "mini" and t.n_buckets == (1 if buckets == "from_items" else 256) and _same_items(t.items(), (codes, counts))
    before = t.data.clone()
    for emit in EMITS:
        abd = t.abundance_of(s, plan, *emit)
        assert t.rows_form == ("find" if find.endswith("1") else "lookup")
        assert np.array_equal(_np(abd), want[emit]) and torch.equal(t.data, before)


@pytest.mark.parametrize("k", _ids(KS))
def test_key_partitioned_pipeline_on_the_same_stream(k):
    """ragged reads together with a Plan in the other pipeline: a bucketed hash table with the lookups inside its count
    (k <= 21), a wide table with the lookup kernel (k > 21)"""
    c = _case(k)
    s, rows, plan = _on_gpu(c.laid)
    for emit in EMITS:
        if k <= 21:
            t = kmer.KmerTable.with_slots(k, DEV, 18, 7).count(s, rows=plan, emit=emit)
            assert t.kind == "hash" and t._emitted == emit
        else:
            t = kmer.count_kmers(s, k, kind="wide")
            assert t.kind == "wide"
        assert _same_items(t.items(), c.items)
        tnf, abd = kmer.features(s, plan, k_tnf=4, table=t, window=emit[0], vsize=emit[1])
        assert np.array_equal(_np(tnf), c.tnf) and np.array_equal(_np(abd), c.abd[emit])
        _, abd_l = kmer.features(s, rows, k_tnf=None, table=t, window=emit[0], vsize=emit[1], seg_chars=32)
        assert np.array_equal(_np(abd_l), c.abd[emit])


# ------------------------------------------------------------------ without the oracle


def _items_and_rows(k, geometry, laid, emit=(10, 400)):
    s, rows, plan = _on_gpu(laid)
    t = _fused(k, geometry, s, plan, emit)
    items = t.items()
    _, abd = kmer.features(s, plan, k_tnf=None, table=t, window=emit[0], vsize=emit[1])
    return items, _np(abd)


def _per_read(laid, abd):
    """the rows of every read added up (a read of the second copy has two)"""
    return np.add.reduceat(abd, np.flatnonzero(np.diff(laid.read_of_row, prepend=-1)))


@pytest.mark.parametrize("k,geometry", CASES)
def test_reverse_complemented_stream_gives_the_same_table(k, geometry):
    """every read reverse complemented, in reverse order: the same canonical k-mers, so the same table; and a read's row is
    the row of its reverse complement (the rows of a read that is cut in two, added up)"""
    reads = _corpus.corpus(k)
    laid = _corpus.stream_of(reads, 0, k)
    back = _corpus.stream_of([_corpus.revcomp(r) for r in reversed(reads)], 0, k)
    assert back.text != laid.text
    items, abd = _items_and_rows(k, geometry, laid)
    items_b, abd_b = _items_and_rows(k, geometry, back)
    assert len(items[0]) > 2000 and _same_items(items_b, items)
    row_of = {}
    for r, row in zip(laid.reads, _per_read(laid, abd)):
        assert np.array_equal(row_of.setdefault(r, row), row)             # (equal reads: equal rows)
    assert all(np.array_equal(row, row_of[_corpus.revcomp(r)]) for r, row in zip(back.reads, _per_read(back, abd_b)))
    assert abd.sum() > 0


@pytest.mark.parametrize("k", _ids(KS))
def test_a_shift_against_the_word_grid_changes_nothing(k):
    """``shift`` N's in front move every read, N and soft-masked base to another position of its word, and the chunk and
    round boundaries to other k-mers: the same table and the same rows as without (odd shifts in the first-pass geometry)"""
    reads = _corpus.corpus(k)
    items, abd = _items_and_rows(k, "both-passes", _corpus.stream_of(reads, 0, k))
    assert len(items[0]) > 2000 and abd.sum() > 0
    for j in (range(1, 32) if k in ALL_SHIFTS else (1, 7, 16, 31)):
        items_j, abd_j = _items_and_rows(k, "first-pass" if j % 2 else "both-passes", _corpus.stream_of(reads, j, k))
        assert _same_items(items_j, items) and np.array_equal(abd_j, abd), j


@pytest.mark.parametrize("cap", [1, 2])
def test_a_smaller_record_cap_changes_nothing(cap):
    """PG_MINI_CAP (read once per process) cuts every run of k-mers under one minimizer after ``cap`` of them: more records,
    the same table and rows -- the fused count of this file at five k, in a process of its own"""
    selection = " or ".join(f"k{k}-" for k in CAP_KS)
    _child(f"test_fused_count_and_lookups and ({selection})", len(CAP_KS) * len(GEOMETRY), PG_MINI_CAP=str(cap))
