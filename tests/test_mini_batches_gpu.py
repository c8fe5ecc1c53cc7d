"""The prefetched-plan batch loop (``KmerTable.prefetch_plan`` + ``count(check=False)`` + ``check_status``) on batches that DIFFER.

One table object and one side stream run a stream of batches in the order of the one-GPU headline loop: reset, count without a
host check, prefetch the next batch's plan, features, check_status.  From the second batch on the count takes the optimistic
branch of ``KmerTable._take_prefetched_plan``: the workspaces of the previous batch, the plan's record counts unread on the host.
The kernels must refuse a batch that does not fit (PG_STATUS_PLAN_MISMATCH, nothing written) and ``check_status`` must count it
again (``KmerTable.recounts``); an accepted batch must give exactly its own table and rows although the record, slot and shuffle
workspaces still hold the batch before.

Reference of every batch, bit for bit: the oracle's table and ``oracle.abd_row`` of every row, and the same batch counted on a
fresh table with its plan computed in front (the host-synchronised path), whose ``plan_counts()`` also give the (records, long
records) that decide what the loop is expected to do.  A k-mer belongs to the row its LAST character lies in (include/
pangaea_feat.h: "the row its k-mer ends in"), so the oracle's row of [a, b) is that of text[a - k + 1 : b].

Which step is refused is derived, not written down: a batch is refused iff its records exceed the record capacity that the last
host-synchronised count left (``kmer._slack`` of its records, rounded as pg_mini_records_bytes does; ``_grown``'s keep-or-replace
rule) -- ``_Sizes`` restates that and is itself checked against the table's buffers after every step.  Every test asserts on its
INPUTS that no batch lies within 1 % of that boundary.

Refusal by the slot buffer alone (S2: the later check of mini_count_kernel, ``wbase + need > mg.cap``, by which time other
workgroups have written their slices).  The slot buffer is pg_mini_merge_words of the sizing batch's counts with slack: per class
(records / 64 + buckets) batches of 64 records -- 128 dwords a batch of short records, 288 a batch of long ones at k = 21 --
where the kernel claims ceil(records of the bucket / 64) batches per bucket.  So a batch's claim lies between its own
pg_mini_merge_words WITHOUT the buckets' frames (``_Sizes.slots_at_least``) and with them (``fits_slots``), and a batch with no
more records but more LONG ones than the sizing batch had can pass the record check and fail this one, provided the frames of
the empty buckets do not swamp the difference: few buckets, many words.  The pair of the issue's hint, H2 then H1 on 2^16
buckets, is not one (``test_slot_buffer_after_h2_holds_h1``: the frames are 27 M dwords in both figures).  S2 runs at 2^15 words
on 512 buckets (two scatter passes): H2 over a prefix of the text -- short records only, about as many as H1 has records --
sizes the buffers, then H1, whose records fit and whose 100 k long records do not.  Every optimistic step derives one of
accepted / refused / refused-slots from these bounds, or fails on its inputs where they do not decide.
"""
import functools
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import oracle
from pangaea_amd import _lib, kmer
from pangaea_amd.reads import ReadStream, Rows

DEV = "cuda:0"
N_WORDS = 4096                      # words of a batch (2^17 characters); at most 2^15
WINDOW, VSIZE = 2, 8

# name, runs [(barcode, text)], rows (Rows), (n_records, n_long) in closed form or None
Batch = namedtuple("Batch", "name runs rows closed")


# ---------------------------------------------------------------------------------------------------------------- batch builders

def _bases(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)


def _runs_and_rows(text: bytes, cuts):
    """the text as runs cut at ``cuts``; every run is a row"""
    edges = [0] + [int(c) for c in cuts] + [len(text)]
    runs = [(f"bc{i}", text[a:b]) for i, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]
    start = np.array(edges[:-1], dtype=np.int64)
    end = np.array(edges[1:], dtype=np.int64)
    return runs, Rows(np.arange(len(runs), dtype=np.int64), [n for n, _ in runs], start, end)


def batch_L(seed: int, k: int, n_words: int = N_WORDS) -> Batch:
    """random A/C/G/T with an N at every (k+1)-th character: every fragment holds exactly one k-mer, hence exactly one record"""
    n = 32 * n_words
    t = _bases(np.random.RandomState(1000 + seed), n)
    t[k::k + 1] = ord("N")
    units = n // (k + 1)
    cuts = [(k + 1) * (units * f // 16) for f in (1, 3, 4, 9)]              # runs of unequal length, each ending in its N
    runs, rows = _runs_and_rows(t.tobytes(), cuts)
    return Batch(f"L{seed}", runs, rows, ((n + 1) // (k + 1), 0))


def batch_Z(kind: str, k: int, n_words: int = N_WORDS) -> Batch:
    """no valid k-mer at all: ``all-n``, or ``short`` -- every fragment one character shorter than k"""
    n = 32 * n_words
    if kind == "all-n":
        t = np.full(n, ord("N"), dtype=np.uint8)
    else:
        t = _bases(np.random.RandomState(77), n)
        t[k - 1::k] = ord("N")
    runs, rows = _runs_and_rows(t.tobytes(), [n // 5, n // 2])
    return Batch(f"Z-{kind}", runs, rows, (0, 0))


def batch_H1(seed: int, n_words: int = N_WORDS) -> Batch:
    """N-free text, rows = whole runs of unequal length: the ordinary mix of short and long records.  Pieces of a quarter-size
    random sequence, so that multiplicities (and the rows' bins) vary."""
    n = 32 * n_words
    rng = np.random.RandomState(2000 + seed)
    genome = _bases(rng, n // 4)
    parts, have = [], 0
    while have < n:
        a = rng.randint(0, len(genome) - 200)
        p = genome[a:a + rng.randint(200, 3000)]
        parts.append(p)
        have += len(p)
    t = np.concatenate(parts)[:n]
    cuts = np.sort(rng.choice(np.arange(1000, n - 1000, 1000), size=6, replace=False) + rng.randint(0, 500))
    runs, rows = _runs_and_rows(t.tobytes(), cuts)
    return Batch(f"H1-{seed}", runs, rows, None)


def batch_H2(seed: int, k: int, n_words: int = N_WORDS, prefix: int | None = None) -> Batch:
    """N-free random text, one-character rows over [k-1, n): every k-mer is its own record.  ``prefix``: bases and rows over the
    first ``prefix`` characters only, N behind them -- prefix - k + 1 short records and nothing else"""
    n = 32 * n_words
    t = _bases(np.random.RandomState(3000 + seed), n)
    m = n if prefix is None else int(prefix)
    t[m:] = ord("N")
    start = np.arange(k - 1, m, dtype=np.int64)
    rows = Rows(np.zeros(len(start), dtype=np.int64), [f"r{i}" for i in range(len(start))], start, start + 1)
    return Batch(f"H2-{seed}" + ("" if prefix is None else f"-first{m}"), [("x", t.tobytes())], rows, (m - k + 1, 0))


def _text(b: Batch) -> bytes:
    return b"".join(t for _, t in b.runs)


def test_batch_builders_on_the_host():
    """no device: equal word counts, the stated N spacing, and the closed-form record counts restated from the text itself
    (a record cannot span a non-base, and a one-character row ends a record at every k-mer)"""
    for k in (15, 21, 27):
        batches = [batch_L(0, k), batch_L(1, k), batch_Z("all-n", k), batch_Z("short", k), batch_H1(0), batch_H1(1), batch_H2(0, k)]
        for b in batches:
            s = ReadStream.from_runs(b.runs, device="cpu")
            assert s.n_words == N_WORDS <= 1 << 15 and s.n_chars == 32 * N_WORDS, b.name
            text = np.frombuffer(_text(b), dtype=np.uint8)
            assert s.decode() == text.tobytes()
            assert (b.rows.end > b.rows.start).all() and (b.rows.start[1:] >= b.rows.end[:-1]).all() and b.rows.end[-1] == len(text)
            is_n = text == ord("N")
            frag = [len(f) for f in text.tobytes().split(b"N")]
            kmers = sum(max(0, f - k + 1) for f in frag)
            if b.name.startswith("L"):
                assert np.array_equal(np.nonzero(is_n)[0], np.arange(k, len(text), k + 1))
                assert all(f == k for f in frag[:-1]) and frag[-1] <= k
                assert b.closed == (sum(f == k for f in frag), 0) and kmers == b.closed[0]      # one k-mer per complete fragment
                assert len(set(np.diff(np.r_[b.rows.start, len(text)]))) > 2                     # runs of unequal length
                assert all(text[e - 1] == ord("N") for e in b.rows.end[:-1])
            elif b.name.startswith("Z"):
                assert kmers == 0 and b.closed == (0, 0) and max(frag) < k
                assert is_n.all() == (b.name == "Z-all-n")
            elif b.name.startswith("H1"):
                assert not is_n.any() and len(b.runs) > 3 and len(set(len(t) for _, t in b.runs)) > 3
            else:
                assert not is_n.any() and b.closed == (kmers, 0) == (len(text) - k + 1, 0)
                assert len(b.rows) == kmers and (b.rows.end - b.rows.start == 1).all() and b.rows.start[0] == k - 1
        assert _text(batches[0]) != _text(batches[1]) and _text(batches[4]) != _text(batches[5])       # other seed, other bases
    assert ReadStream.from_runs(batch_H1(0, N_WORDS // 2).runs, device="cpu").n_words == N_WORDS // 2
    # S2's batches: 2^15 words each; the partial H2 has its k-mers in the prefix only
    for make, args in _s2(21):
        b = make(*args)
        assert ReadStream.from_runs(b.runs, device="cpu").n_words == S2_WORDS == 1 << 15, b.name
    b = batch_H2(1, 21, S2_WORDS, S2_PREFIX)
    text = _text(b)
    assert text[S2_PREFIX:] == b"N" * (32 * S2_WORDS - S2_PREFIX) and b"N" not in text[:S2_PREFIX]
    assert b.closed == (S2_PREFIX - 21 + 1, 0) and len(b.rows) == b.closed[0] and b.rows.end[-1] == S2_PREFIX


# -------------------------------------------------------------------------------------------------------------------- references

@functools.lru_cache(maxsize=None)
def _oracle(make, args, k: int):
    """(batch, sorted codes, counts, abundance rows of ALL rows) -- computed once per batch and k, shared, never changed"""
    b = make(*args)
    text = _text(b)
    table = oracle.Table(k, threads=4).count(text)
    codes, counts = table.items()
    abd = np.stack([oracle.abd_row(text[max(0, a - k + 1):e], k, table, WINDOW, VSIZE) for a, e in zip(b.rows.start, b.rows.end)])
    for x in (codes, counts, abd):
        x.setflags(write=False)
    return b, codes, counts, abd


Prepared = namedtuple("Prepared", "batch stream plan codes counts abd n_records n_long fresh_abd")


def _prepare(spec, k, log2_slots, log2_bucket, with_rows=True) -> Prepared:
    """the batch on the device, the oracle's answers, and the host-synchronised answers of a FRESH table (plan in front)"""
    make, args = spec
    b, codes, counts, abd = _oracle(make, args, k)
    s = ReadStream.from_runs(b.runs, device=DEV)
    plan = kmer.Plan(b.rows, DEV) if with_rows else None
    t = kmer.KmerTable.mini_with_slots(k, DEV, log2_slots, log2_bucket)
    t.count(s, rows=plan, emit=(WINDOW, VSIZE) if with_rows else None)
    assert t._mini_plan.n_records is not None and t.recounts == 0              # the plan in front: counts read on the host
    n_records, n_long = t.plan_counts()
    if b.closed is not None and (with_rows or not b.name.startswith("H2")):
        assert (n_records, n_long) == b.closed, (b.name, n_records, n_long)     # mini_plan_kernel against the closed form
    if t.kind == "mini":
        counts = np.minimum(counts, np.uint64(_lib.HASH_COUNT_SAT))
    _assert_items(t, codes, counts, b.name + " on a fresh table")
    fresh = None
    if with_rows:
        fresh = kmer.features(s, plan, k_tnf=None, table=t, window=WINDOW, vsize=VSIZE)[1].cpu()
        assert np.array_equal(fresh.numpy(), abd), b.name + " on a fresh table: rows"
    print(f"    {b.name}: n_words {s.n_words} (n_records, n_long) = ({n_records}, {n_long})")
    return Prepared(b, s, plan, codes, counts, abd, n_records, n_long, fresh)


def _assert_items(t, codes, counts, what):
    got = t.items()
    assert np.array_equal(got[0], codes) and np.array_equal(got[1], counts), f"{what}: items() differ from the oracle's"


class _Sizes:
    """what ``KmerTable`` keeps of record and slot workspaces from count to count, restated from ``kmer._slack``, the library's
    own size functions and ``_grown``'s rule -- the expectation of 'refused' comes from here"""

    def __init__(self, t, merged: bool, host_sync: bool):
        self.t, self.merged, self.host_sync = t, merged, host_sync
        self.rec_bytes = self.slot_words = self.sized_for = None

    def _words(self, n_words, n_records, n_long):
        return _lib.check(_lib.load().pg_mini_merge_words(n_words, n_records, n_long, self.t.desc()))

    @property
    def rec_cap(self):                                       # records (8-byte bases x 2, 4-byte meta x 2), a multiple of 256
        return self.rec_bytes // 24 // 256 * 256

    def path(self, i: int, p: Prepared) -> str:
        """front: no prefetched plan; host: a prefetched plan, its counts read on the host; optimistic: accepted, refused (by the
        record count: every kernel returns before it writes) or refused-slots (by the slot buffer alone, in the count kernel)"""
        if i == 0:
            return "front"
        if self.host_sync or self.sized_for != p.stream.n_words:
            return "host"
        # (a condition on the inputs: no batch within 1 % of a boundary)
        assert abs(p.n_records - self.rec_cap) > 0.01 * self.rec_cap, (p.batch.name, p.n_records, self.rec_cap)
        if p.n_records > self.rec_cap:
            return "refused"
        if self.fits_slots(p):
            return "accepted"
        low = self.slots_at_least(p)
        print(f"    {p.batch.name}: slot dwords kept {self.slot_words}, claimed at least {low}, at most {self._words(p.stream.n_words, p.n_records, p.n_long)}")
        assert self.slot_check(p) and low > 1.01 * self.slot_words, (p.batch.name, "the slot bounds do not decide", low, self.slot_words)
        return "refused-slots"

    def slot_check(self, p: Prepared) -> bool:
        """does the count kernel of this batch check a slot buffer at all (the library's own rule for the merged lookups)?"""
        return self.merged and p.plan is not None and _lib.check(_lib.load().pg_mini_merge_form_applies(self.t.desc(), p.plan.n_rows, VSIZE)) == 1

    def slots_at_least(self, p: Prepared) -> int:
        """a lower bound of what the batch's buckets claim together: pg_mini_merge_words of its counts without the frame of every
        bucket (the figure for no records at all) and without the rounding to 256 -- sum of ceil(x_b / 64) >= floor(sum x_b / 64)"""
        n = p.stream.n_words
        return self._words(n, p.n_records, p.n_long) - self._words(n, 0, 0) - 256

    def fits_slots(self, p: Prepared) -> bool:
        """pg_mini_merge_words of the batch's own counts bounds what its buckets claim (per class records / 64 + buckets batches,
        the kernel claims ceil(records of the bucket / 64) per bucket; a step's slack in both): at or below the kept buffer the slot
        buffer cannot be what refuses the batch"""
        return not self.slot_check(p) or self._words(p.stream.n_words, p.n_records, p.n_long) <= self.slot_words

    def host_sized(self, p: Prepared) -> None:
        """a count that read its plan's counts on the host (in front, host-synchronised, or a recount)"""
        need = _lib.check(_lib.load().pg_mini_records_bytes(kmer._slack(p.n_records), self.t.desc()))
        if self.rec_bytes is None or self.rec_bytes < need or self.rec_bytes > 2 * need:
            self.rec_bytes = need
        if self.merged:
            s = kmer._slack(p.n_records)
            self.slot_words = max(self.slot_words or 0, self._words(p.stream.n_words, s, min(kmer._slack(p.n_long), s)))
        self.sized_for = p.stream.n_words

    def check(self) -> None:
        assert self.t._mini_rec_ws.numel() == self.rec_bytes
        assert not self.merged or self.t._merge_ws.numel() == self.slot_words


def _loop(specs, k, log2_slots, log2_bucket, expect, after=None, with_rows=True):
    """the loop under test; ``expect``: the paths the sequence is MEANT to take (the derived ones must agree: a sequence that
    no longer does what its name says fails instead of passing on another path).  Returns the table."""
    assert len(specs) <= 7
    refused = ("refused", "refused-slots")
    merged = with_rows and kmer._merged_lookups()
    host_sync = os.environ.get("PG_PLAN_HOST_SYNC", "0") not in ("", "0")
    batches = [_prepare(sp, k, log2_slots, log2_bucket, with_rows) for sp in specs]
    t = kmer.KmerTable.mini_with_slots(k, DEV, log2_slots, log2_bucket)
    sizes = _Sizes(t, merged, host_sync)
    side = torch.cuda.Stream(device=DEV)
    emit = (WINDOW, VSIZE) if with_rows else None
    taken, ahead_ws = [], None
    for i, p in enumerate(batches):
        what = f"step {i} ({p.batch.name})"
        path = sizes.path(i, p)
        taken.append(path)
        before = t.recounts
        event = None
        if after == "event":
            event = torch.cuda.Event()
            event.record()                                               # before the count: the next plan runs beside it
        t.reset()
        t.count(p.stream, check=False, rows=p.plan, emit=emit)
        # (i) the path, right after the count
        assert (t._mini_plan.n_records is None) == (path in ("accepted",) + refused), what
        if i:
            assert t._mini_next is None and t._mini_plan.ws is ahead_ws, what + ": the prefetched plan was not the one used"
        if i + 1 < len(batches):
            nxt = batches[i + 1]
            t.prefetch_plan(nxt.stream, nxt.plan, side, after=event if after == "event" else after)
            ahead_ws = t._mini_next.ws
        rows = None
        if with_rows and path not in refused:
            rows = kmer.features(p.stream, p.plan, k_tnf=None, table=t, window=WINDOW, vsize=VSIZE)[1]
        t.check_status()
        # (ii) the table
        _assert_items(t, p.codes, p.counts, what + f" [{path}]")
        assert t.recounts - before == (1 if path in refused else 0), what + f" [{path}]: recounts moved by {t.recounts - before}"
        if path != "accepted":
            sizes.host_sized(p)
        sizes.check()
        # (iii) the rows
        if with_rows:
            if path in refused:
                rows = kmer.features(p.stream, p.plan, k_tnf=None, table=t, window=WINDOW, vsize=VSIZE)[1]
            rows = rows.cpu()
            assert np.array_equal(rows.numpy(), p.abd), what + f" [{path}]: rows differ from the oracle's"
            assert torch.equal(rows, p.fresh_abd), what + f" [{path}]: rows differ from a fresh table's"
            if p.n_records == 0:
                assert not rows.any() and len(p.codes) == 0
    print("    paths:", " ".join(taken))
    assert taken == list(expect), taken
    return t


def _s1(k, z="short"):
    """L0 (plan in front, small) -> L1 (accepted: same count, other bases) -> H1 (refused) -> L2 (accepted, H1's data behind it)
    -> Z (accepted: empty table, all-zero rows) -> H1' (accepted) -> H2 (refused again)"""
    return [(batch_L, (0, k)), (batch_L, (1, k)), (batch_H1, (0,)), (batch_L, (2, k)), (batch_Z, (z, k)), (batch_H1, (1,)), (batch_H2, (0, k))]


S2_WORDS = 1 << 15
# H1 at 2^15 words and k = 21 has 8 x (29.3 k records, 12.5 k long ones) = 235 k and 100 k.  A sizing batch of 228 k short records
# leaves a record capacity of 239.6 k (H1 fits, 2 % below) and a slot buffer of 2.0625 x 228 k + 4.5 x 4096 dwords + the buckets'
# frames, which H1's 2 x 134 k + 4.5 x 100 k dwords exceed by 2 % before any bucket has rounded up.  (_Sizes.path asserts both.)
S2_PREFIX = 228_000 + 20


def _s2(k):
    """partial H2 (plan in front: short records only) -> H1 (records fit, slot words do not: refused by the count kernel, after
    other buckets have written) -> L (accepted in the new buffers) -> H1' (accepted: the slot buffer is H1's now)"""
    return [(batch_H2, (1, k, S2_WORDS, S2_PREFIX)), (batch_H1, (0, S2_WORDS)), (batch_L, (0, k, S2_WORDS)), (batch_H1, (1, S2_WORDS))]


S1_PATHS = ["front", "accepted", "refused", "accepted", "accepted", "accepted", "refused"]


# --------------------------------------------------------------------------------------------------------------------- the tests

@pytest.mark.gpu
def test_batch_loop_through_the_checked_build():
    """FIRST in this file: every other GPU test of it in a process of its own on the library built with -DPG_CHECKED (a store
    outside its buffer becomes PG_STATUS_BOUNDS instead of a memory fault), before the product build runs them"""
    if os.environ.get("PANGAEA_LIB") == "checked":
        pytest.skip("already inside the checked pass")
    from .conftest import ROOT
    env = dict(os.environ, PANGAEA_LIB="checked", PG_MINI_MERGE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_mini_batches_gpu.py"),
                        "-k", "not through_the_checked_build"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("k,log2_slots,log2_bucket,z", [
    (21, 22, 10, "short"),        # both scatter passes
    (21, 19, 14, "short"),        # first pass only, 1024-thread workgroups
    (21, 24, 8, "short"),         # 2^16 buckets
    (15, 20, 10, "all-n"),        # 11-mer minimizers
    (27, 20, 11, "all-n"),        # miniw: prefetch_plan applies to it too
])
def test_s1_accepted_and_refused_batches_in_reused_workspaces(k, log2_slots, log2_bucket, z):
    t = _loop(_s1(k, z), k, log2_slots, log2_bucket, S1_PATHS)
    assert t.recounts == 2


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["event", "first-pass", "host-sync", "word-wise"])
def test_s1_other_wait_points_and_forms(form, monkeypatch):
    """``after=`` an event recorded before the count, ``after="first-pass"`` (pg_mini_wait_first_pass), PG_PLAN_HOST_SYNC=1 (nothing
    is optimistic: every prefetched plan's counts are read on the host, no recount), PG_MINI_MERGE=0 (no slot buffer)"""
    if form == "host-sync":
        monkeypatch.setenv("PG_PLAN_HOST_SYNC", "1")
    if form == "word-wise":
        monkeypatch.setenv("PG_MINI_MERGE", "0")
    after = form if form in ("event", "first-pass") else None
    expect = ["front"] + ["host"] * 6 if form == "host-sync" else S1_PATHS
    t = _loop(_s1(21), 21, 22, 10, expect, after=after)
    assert t.recounts == (0 if form == "host-sync" else 2)
    assert (t._merge_ws is None) == (form == "word-wise")


@pytest.mark.gpu
def test_s2_refused_by_the_slot_buffer_alone():
    """512 buckets, two scatter passes.  The expectation is derived on the host from pg_mini_merge_words (``_Sizes.path``) before
    the loop counts the batch; what the bounds were is printed."""
    t = _loop(_s2(21), 21, 20, 11, ["front", "refused-slots", "accepted", "accepted"])
    assert t.recounts == 1


@pytest.mark.gpu
def test_s3_a_batch_of_another_size_in_the_middle():
    """a batch of half the words takes the host-synchronised branch (``_mini_sized_for`` differs), and so does the first batch
    back at the original size; the one after that is optimistic again -- and refused, the record buffer being the half-size
    batch's (``_grown`` keeps a buffer that is less than twice too large)"""
    k = 21
    specs = [(batch_L, (0, k)), (batch_L, (1, k)), (batch_H1, (0, N_WORDS // 2)), (batch_L, (2, k)), (batch_H1, (1,)), (batch_L, (3, k))]
    t = _loop(specs, k, 22, 10, ["front", "accepted", "host", "host", "refused", "accepted"])
    assert t.recounts == 1


@pytest.mark.gpu
def test_s4_table_only():
    """S1's first four batches without rows and without lookups: the record buffers alone"""
    t = _loop(_s1(21)[:4], 21, 22, 10, S1_PATHS[:4], with_rows=False)
    assert t.recounts == 1 and t._merge_ws is None


@pytest.mark.gpu
def test_rows_taken_before_check_status_of_a_refused_batch_are_void_and_recounts_says_so():
    """the headline loop's order on a batch refused by its record count (every kernel returns before it writes): features() has
    run on a count that counted nothing when check_status() silently counts again.  ``recounts`` is what tells the caller; the
    rows taken afterwards are the oracle's.  (The first rows are not compared with anything.)"""
    k = 21
    small, big = _prepare((batch_L, (0, k)), k, 22, 10), _prepare((batch_H1, (0,)), k, 22, 10)
    t = kmer.KmerTable.mini_with_slots(k, DEV, 22, 10)
    sizes = _Sizes(t, kmer._merged_lookups(), False)
    side = torch.cuda.Stream(device=DEV)
    t.count(small.stream, check=False, rows=small.plan, emit=(WINDOW, VSIZE))
    t.prefetch_plan(big.stream, big.plan, side)
    kmer.features(small.stream, small.plan, k_tnf=None, table=t, window=WINDOW, vsize=VSIZE)
    t.check_status()
    sizes.host_sized(small)
    assert sizes.path(1, big) == "refused" and t.recounts == 0
    t.reset()
    t.count(big.stream, check=False, rows=big.plan, emit=(WINDOW, VSIZE))
    assert t._mini_plan.n_records is None
    kmer.features(big.stream, big.plan, k_tnf=None, table=t, window=WINDOW, vsize=VSIZE)          # void
    t.check_status()
    _assert_items(t, big.codes, big.counts, "the refused batch after check_status")
    assert t.recounts == 1
    again = kmer.features(big.stream, big.plan, k_tnf=None, table=t, window=WINDOW, vsize=VSIZE)[1].cpu()
    assert np.array_equal(again.numpy(), big.abd) and torch.equal(again, big.fresh_abd)
    t.check_status()
    assert t.recounts == 1


@pytest.mark.gpu
def test_slot_buffer_after_h2_holds_h1():
    """why the pair one would try first, a full H2 then H1 on 2^16 buckets, is NOT refused by the slot buffer alone (S2 uses
    another pair: see the head of this file): by pg_mini_merge_words itself the buffer that H2 sizes holds even the upper bound of
    what H1 claims -- the frames of the 2^16 buckets are in both figures and make up nearly all of them"""
    k = 21
    h2, h1 = _prepare((batch_H2, (0, k)), k, 24, 8), _prepare((batch_H1, (0,)), k, 24, 8)
    t = kmer.KmerTable.mini_with_slots(k, DEV, 24, 8)
    sizes = _Sizes(t, True, False)
    sizes.host_sized(h2)
    assert h1.n_records <= sizes.rec_cap and sizes.fits_slots(h1)
    own = sizes._words(N_WORDS, h1.n_records, h1.n_long)
    print(f"    slot dwords: kept after H2 {sizes.slot_words}, H1's own bound {own}")
    assert own < sizes.slot_words
