"""The plan kernel and the first scatter pass with the per-position forms of mini_forms.hpp, on a stream of two chunks and one word.

580 reads laid out three times by ``_corpus.stream_of`` (in order, reversed with every read cut into two rows, permuted): 1740 reads,
about 870 pairs of 150 bp, 8193 words -- two whole 4096-word chunks and a chunk of a single word.  Reads drawn from a short
genome (multiplicities vary), every ninth with an N at a position of its own, a poly-A read, a read shorter than every k; one
row per read (two in the second copy), so rows begin and end inside words.

At k = 13, 15, 16, 21, 22, 31 (11- and 13-mers, windows of 3, 5, 4, 9, the delayed windows of 8 and 9): the table and the
abundance rows of a count with the lookups inside are the oracle's; ``plan_counts()`` -- what mini_plan_kernel counted -- equals
the records counted in Python (``_corpus.count_records``) AND the records the first pass wrote (the entries of its meta plane
that are no longer the fill value), with PG_STATUS_PLAN_MISMATCH clear; the same with the plan computed by ``prefetch_plan`` on a
side stream; and pg_mini_plan_masked on the same stream with a quality plane against the Python count under the masked rule,
followed (k <= 21) by the masked count half, whose first pass checks the masked plan.  Everything runs through the checked build
first, in a process of its own."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import oracle
from pangaea_amd import _lib, kmer
from pangaea_amd.reads import ReadStream

from . import _corpus
from .conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = (13, 15, 16, 21, 22, 31)
EMIT = (10, 400)
N_WORDS = 2 * 4096 + 1
GEOMETRY = {"first-pass": (18, 10), "both-passes": (20, 10)}      # 2^8 buckets: the first pass alone; 2^10: both passes
FILL = 0xFF                                                         # no meta word is 0xFFFFFFFF: a record holds at most 9 k-mers


def _reads():
    rng = np.random.RandomState(4711)
    genome = _corpus._random(rng, 20_000)
    reads = []
    for i in range(577):
        a = rng.randint(0, len(genome) - 150)
        r = genome[a:a + 150]
        if i % 9 == 4:
            p = (17 * i) % 150
            r = r[:p] + b"N" + r[p + 1:]
        reads.append(r)
    reads.insert(100, b"A" * 150)
    reads.insert(300, genome[7:19])                                 # 12 characters: shorter than every k
    reads.insert(500, genome[1000:1095])                            # (brings the three copies to 8193 words)
    return reads


@functools.lru_cache(maxsize=None)
def _laid():
    laid = _corpus.stream_of(_reads(), 0)
    assert laid.n_words == N_WORDS and len(laid.reads) == 1740
    assert b"A" * 150 in laid.reads and min(len(r) for r in laid.reads) == 12 < min(KS)
    assert sum(b"N" in r for r in laid.reads) == 3 * 64
    assert {int(x) % 32 for x in laid.start} == set(range(32)) == {int(x) % 32 for x in laid.end}
    return laid


@functools.lru_cache(maxsize=None)
def _case(k):
    """what the oracle and the Python record count say about the stream at this k; shared, never written to"""
    laid = _laid()
    table = oracle.Table(k, threads=4).count(laid.text)
    abd = laid.rows_by_oracle(lambda seq: oracle.abd_row(seq, k, table, *EMIT)).astype(np.int32)
    assert abd.sum() > 0
    return SimpleNamespace(k=k, laid=laid, items=table.items(), abd=abd, records=_corpus.count_records(laid, k))


def _on_gpu():
    laid = _laid()
    s = ReadStream.from_runs(laid.runs, device=DEV)
    assert s.n_words >= N_WORDS and s.n_chars == len(laid.text)
    return s, kmer.Plan(laid.rows(), DEV)


def _first_pass_records(t):
    """records in the first pass's meta plane: the record workspace is two planes of 8-byte bases, then two of 4-byte meta words"""
    ws = t._mini_rec_ws
    cap = ws.numel() // 24 // 256 * 256
    assert _lib.check(_lib.load().pg_mini_records_meta_offset(ws.numel(), t.desc())) == 20 * cap
    meta_a = ws[16 * cap:20 * cap].view(torch.int32)
    return int((meta_a != -1).sum().item())


def _check_count(c, t, s, plan):
    assert t.recounts == 0 and int(t.status[0].item()) == 0                       # (PG_STATUS_PLAN_MISMATCH among them)
    assert t.plan_counts() == c.records
    assert _first_pass_records(t) == c.records[0]
    got = t.items()
    assert np.array_equal(got[0], c.items[0]) and np.array_equal(got[1], c.items[1])
    _, abd = kmer.features(s, plan, k_tnf=None, table=t, window=EMIT[0], vsize=EMIT[1])
    assert np.array_equal(abd.cpu().numpy(), c.abd)


def _counted_into_filled_workspace(k, geometry, s, plan, prefetch):
    """a count whose record workspace held nothing but FILL bytes when the first pass wrote into it: the first count sizes the
    workspace, the second -- after reset(), on the same plan or on one that ``prefetch_plan`` computed on a side stream -- reuses it"""
    t = kmer.KmerTable.mini_with_slots(k, DEV, *GEOMETRY[geometry])
    t.count(s, rows=plan, emit=EMIT)
    ws = t._mini_rec_ws
    ws.fill_(FILL)
    t.reset()
    if prefetch:
        t._mini_plan = None                                                       # (forget the plan in use: the next one comes from the side stream)
        t.prefetch_plan(s, plan, torch.cuda.Stream(device=DEV))
        assert t._mini_next is not None
    t.count(s, check=False, rows=plan, emit=EMIT)
    assert t._mini_next is None and t._mini_rec_ws is ws
    t.check_status()
    return t


def test_through_the_checked_build_first():
    if os.environ.get("PANGAEA_LIB") == "checked":
        pytest.skip("already inside the checked pass")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_plan_forms_gpu.py"),
                        "-k", "not through_the_checked_build"], cwd=ROOT, env=dict(os.environ, PANGAEA_LIB="checked"),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("geometry", list(GEOMETRY))
@pytest.mark.parametrize("k", KS)
def test_table_rows_and_record_counts(k, geometry):
    c = _case(k)
    s, plan = _on_gpu()
    _check_count(c, _counted_into_filled_workspace(k, geometry, s, plan, prefetch=False), s, plan)


@pytest.mark.parametrize("k", KS)
def test_plan_prefetched_on_a_side_stream(k):
    c = _case(k)
    s, plan = _on_gpu()
    _check_count(c, _counted_into_filled_workspace(k, "both-passes", s, plan, prefetch=True), s, plan)


# ------------------------------------------------------------------ the masked plan

def _masked(k):
    """the stream with a quality plane: every 23rd base of every third read is below the threshold (never an N).  Returns the
    stream, the (kept, T, R) planes of the masked rule and the Python record count under it"""
    laid = _laid()
    text = np.frombuffer(laid.text, dtype=np.uint8)
    lowq = np.zeros(len(text), dtype=bool)
    off = 0
    for i, r in enumerate(laid.reads):
        if i % 3 == 1:
            lowq[off + 5:off + len(r):23] = True
        off += len(r) + 1
    lowq &= text != ord("N")
    assert lowq.sum() > 3000
    masked = _corpus.MaskedLaid(laid.runs, laid.text, laid.names, laid.start, laid.end, laid.reads, laid.read_of_row, laid.read_start, lowq)
    kept, in_table, in_rows, _ = _corpus.kmer_planes(masked.text, masked.table_text(), masked.start, masked.end, k)
    s = ReadStream.from_runs(laid.runs, device=DEV)
    s.valid_lowq = _corpus.plane_of(lowq, s.n_words).to(DEV)
    # (the quality plane takes k-mers from the table that the rows keep: records of both kinds, cut where the kind changes)
    assert 0 < in_table.sum() < in_rows.sum() and (kept & ~in_table).any()
    return s, _corpus.count_records(masked, k, planes=(kept, in_table, in_rows))


@pytest.mark.parametrize("k", KS)
def test_masked_plan_on_a_stream_with_a_quality_plane(k):
    s, records = _masked(k)
    assert records[0] > 0
    plan = kmer.Plan(_laid().rows(), DEV)
    t = kmer.KmerTable.mini_with_slots(k, DEV, 19, 10)                           # 2^9 buckets: more than 256, as the count half needs
    assert kmer.KmerTable.half_masked(s)
    L = _lib.load()
    ws = torch.empty(_lib.check(L.pg_mini_plan_bytes(s.n_words, t.desc())), dtype=torch.uint8, device=DEV)
    rows_ref = t._rows_ref(plan, s, True)                                       # (the strict plane rides along)
    _lib.check(L.pg_mini_plan_masked(s.codes.data_ptr(), s.union_valid(False).data_ptr(), s.table_valid(False).data_ptr(), 0, s.n_words,
                                     t.desc(), rows_ref, ws.data_ptr(), ws.numel(), kmer._stream_ptr(torch.device(DEV))))
    assert kmer._plan_head(ws) == records
    if k <= 21:
        # the masked first pass ends every (chunk, region) run where the masked plan put the next one, or says so
        t.count_half(s, plan, EMIT, check=False)
        assert int(t.status[0].item()) == 0 and t.recounts == 0 and t.plan_counts() == records
