"""The super-k-mer form on N > 1 ranks (dist.MiniSharded, dist.features_sharded_mini) on the edge-case corpus of tests/_corpus.py,
plain and masked, at every k from 13 to 21.

The other multi-rank tests feed these kernels -- the count half and its pieces, pg_mini_gather_entries, the owner merge, the
lookup half, and the MASKED twins of plan, count half and merge -- with ``synth.generate``: 150-character reads, low-quality bases
at random.  Here a rank's shard holds reads shorter than k, a low-quality base at every position of three words, records that
must be cut because only the table's plane changes, row boundaries inside masked records, reads without a row, row-only k-mers
whose owner holds them from another rank only, from the same rank too, or from nobody, and the all-A k-mer (code 0) row-only on
some ranks and counted on exactly one.  tests/test_mini_corpus_host.py checks on the CPU that the layouts do hold all that.

Ranks share cuda:0 over gloo, as in test_dist_gloo.py; all k of a case go through ONE spawn (the start of the processes is most
of such a test's time), every rank writes an .npz, the parent compares.  Integer results, compared bit for bit with the
project's CPU oracle: the owners' ``owned_items()`` together == ``oracle.Table`` of the table's text; the ranks' TNF and abundance
rows in rank order == ``oracle.tnf_row`` / ``oracle.abd_row`` of the strict text against that table (``Laid.rows_by_oracle``), for
(window, vsize) = (1, 64) and (10, 400) as in test_mini_corpus_gpu.py; every rank's record count == a count in Python under the
masked rule (``_corpus.count_records`` with planes).  Every worker also counts a second time with the same object.  The plain
and the quality-masked case go through the checked build first."""
import dataclasses
import functools
import os
import socket
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import oracle
from pangaea_amd import dist as pdist
from pangaea_amd import kmer

from . import _corpus
from .conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = tuple(range(13, 22))
THREE_KS = (13, 16, 21)                     # minimizers of 11 (k < 16) and of 13; the shortest and the longest window
EMITS = ((1, 64), (10, 400))
WORLDS = [pytest.param(2, id="world2"), pytest.param(3, id="world3")]
PIECE_WORDS = 256
# case -> (the masked layout?, lowercase_is_base)
CASES = {"plain": (False, False), "qual": (True, False), "soft": (True, True), "mixed": (True, False)}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _has_quality(case, rank):
    """"mixed": rank 1's shard comes without a quality plane, so its count half takes the plain form"""
    return CASES[case][0] and not (case == "mixed" and rank == 1)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _worker(rank, world, port, outdir, cases, ks, pieces):
    _init(rank, world, port)
    try:
        out = {}
        for case in cases:
            masked, lc = CASES[case]
            for k in ks:
                sh = _corpus.shard(_corpus.sharded_layout(k, masked), world, rank, quality=_has_quality(case, rank))
                part = sh.stream.to(DEV)
                assert kmer.KmerTable.half_masked(part, lc) == _has_quality(case, rank)
                plan = kmer.Plan(sh.rows, DEV)
                assert plan.shuffle_ok
                for window, vsize in EMITS:
                    tnf, abd, ms = pdist.features_sharded_mini(part, plan, k, 4, window, vsize, lowercase_is_base=lc)
                    assert isinstance(ms, pdist.MiniSharded) and ms.masked == masked and ms.pieces == 1
                    assert ms.local.k == ms.union.k == k and ms.local.n_buckets == ms.union.n_buckets >= 512
                    c, n = ms.owned_items()
                    tag = f"{case}.k{k}.w{window}"
                    out.update({f"{tag}.c": c, f"{tag}.n": n, f"{tag}.tnf": tnf.cpu().numpy(), f"{tag}.abd": abd.cpu().numpy(),
                                f"{tag}.records": np.array(ms.local.plan_counts()[0])})
                    # counting again with the same object gives the same table and rows
                    ms.count(part, plan)
                    _, abd2 = kmer.features(part, plan, k_tnf=None, table=ms.local, window=window, vsize=vsize)
                    assert torch.equal(abd2, abd) and _same(ms.owned_items(), (c, n))
                    del ms
                    if not pieces:
                        continue
                    # the same in pieces of 256 words: reads across every seam; the table and the rows of ONE piece
                    os.environ["PANGAEA_MINI_PIECE_WORDS"] = str(PIECE_WORDS)
                    try:
                        tnf_p, abd_p, mp_ = pdist.features_sharded_mini(part, plan, k, 4, window, vsize, lowercase_is_base=lc)
                        assert mp_.masked == masked and mp_.pieces == -(-part.n_words // PIECE_WORDS) and mp_.pieces >= 8
                        assert _same(mp_.owned_items(), (c, n)) and torch.equal(abd_p, abd) and torch.equal(tnf_p, tnf)
                        mp_.count(part, plan)
                        _, abd2 = kmer.features(part, plan, k_tnf=None, table=mp_.local, window=window, vsize=vsize)
                        assert mp_.pieces >= 8 and torch.equal(abd2, abd) and _same(mp_.owned_items(), (c, n))
                        out[f"{tag}.pieces"] = np.array(mp_.pieces)
                        del mp_
                    finally:
                        del os.environ["PANGAEA_MINI_PIECE_WORDS"]
                out[f"{case}.k{k}.names"] = np.array(sh.rows.names)
        np.savez(os.path.join(outdir, f"c{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _expected(case, k):
    """the layout of a case at this k and everything the oracle says about it; shared by the tests, never written to"""
    masked, lc = CASES[case]
    laid = _corpus.sharded_layout(k, masked)
    if case == "mixed":                                          # rank 1 of 2 has no quality plane: its marks do not exist
        laid = dataclasses.replace(laid, lowq=laid.lowq & (np.arange(len(laid.text)) < _corpus.run_cuts(laid, 2)[1]))
    table_text = laid.table_text(lc) if masked else laid.text
    table = oracle.Table(k, threads=4).count(table_text)
    _corpus.check_against_oracle(laid, k, table)
    e = SimpleNamespace(laid=laid, items=table.items(), table_text=table_text,
                        tnf=laid.rows_by_oracle(lambda seq: oracle.tnf_row(seq, 4)).astype(np.int32),
                        abd={emit: laid.rows_by_oracle(lambda seq: oracle.abd_row(seq, k, table, *emit)).astype(np.int32) for emit in EMITS})
    assert 0 < e.abd[(1, 64)].sum() < e.abd[(10, 400)].sum()
    if masked:
        # (not vacuous: the rows hold k-mers that the table lacks, and the rows against the strict text's own table differ)
        strict = oracle.Table(k, threads=4).count(laid.text)
        assert not np.array_equal(e.abd[(10, 400)], laid.rows_by_oracle(lambda seq: oracle.abd_row(seq, k, strict, 10, 400)))
        assert (0 in e.items[0]) and any(b"A" * k in laid.text[a:b] for a, b in zip(laid.start, laid.end))
    return e


@functools.lru_cache(maxsize=None)
def _records(case, k, world):
    """per rank: the records of its shard, counted in Python (plain: the strict plane alone; masked: kept k-mers, cut where T or R
    changes)"""
    masked, lc = CASES[case]
    laid = _expected(case, k).laid
    out = []
    for rank in range(world):
        sh = _corpus.shard(laid, world, rank)
        own = SimpleNamespace(text=sh.text, start=sh.rows.start, end=sh.rows.end)
        planes = _corpus.kmer_planes(sh.text, sh.table_text(lc), sh.rows.start, sh.rows.end, k)[:3] if masked else None
        out.append(_corpus.count_records(own, k, planes=planes)[0])
    return out


def _run(tmp_path, world, cases, ks, pieces=False):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), tuple(cases), tuple(ks), pieces), nprocs=world, join=True)
    parts = [np.load(str(tmp_path / f"c{r}.npz")) for r in range(world)]
    for case in cases:
        for k in ks:
            e = _expected(case, k)
            assert [n for p in parts for n in p[f"{case}.k{k}.names"].tolist()] == e.laid.names, (case, k)
            for emit in EMITS:
                tag = f"{case}.k{k}.w{emit[0]}"
                # the owners' ranges together are the oracle's table of the table text: counted k-mers only, none of count 0
                codes, counts = (np.concatenate([p[f"{tag}.{x}"] for p in parts]) for x in "cn")
                order = np.argsort(codes, kind="stable")
                assert counts.min() > 0 and _same((codes[order], counts[order]), e.items), tag
                assert np.array_equal(np.concatenate([p[f"{tag}.tnf"] for p in parts]), e.tnf), tag
                assert np.array_equal(np.concatenate([p[f"{tag}.abd"] for p in parts]), e.abd[emit]), tag
                assert [int(p[f"{tag}.records"]) for p in parts] == _records(case, k, world), tag
                if pieces:
                    assert all(int(p[f"{tag}.pieces"]) >= 8 for p in parts), tag
    return parts


# ------------------------------------------------------------------ the checked build first


def test_plain_and_quality_masked_through_the_checked_build_first():
    """the same library built with -DPG_CHECKED (every global store of the super-k-mer kernels checks its index against the
    capacity of its buffer): the plain and the quality-masked case of this file on two ranks run through it in a process of their
    own before anything here runs on the product -- a wrong index shows as PG_STATUS_BOUNDS, which MiniSharded.any_full raises on
    every rank, instead of as a memory fault"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_dist_corpus_gpu.py"),
                        "-k", "(test_plain_on_several_ranks or test_quality_masked_on_several_ranks) and world2"],
                       cwd=ROOT, env=dict(os.environ, PANGAEA_LIB="checked"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ------------------------------------------------------------------ against the oracle


@functools.lru_cache(maxsize=None)
def _one_process(k):
    """the rows ONE process gives for the whole plain stream: count_kmers with the rows emitted, then features"""
    laid = _expected("plain", k).laid
    s = _corpus.host_stream(laid).to(DEV)
    plan = kmer.Plan(laid.rows(), DEV)
    out = {}
    for emit in EMITS:
        t = kmer.count_kmers(s, k, rows=plan, emit=emit)
        tnf, abd = kmer.features(s, plan, k_tnf=4, table=t, window=emit[0], vsize=emit[1])
        out[emit] = (tnf.cpu().numpy(), abd.cpu().numpy())
    return out


@pytest.mark.parametrize("world", WORLDS)
def test_plain_on_several_ranks(tmp_path, world):
    """the plain count half, pg_mini_gather_entries, pg_mini_merge_bins and the lookup half on the unmasked corpus, every k: the
    table, the rows, the records; and the rows one process gives for the whole stream"""
    parts = _run(tmp_path, world, ["plain"], KS)
    for k in KS:
        for emit, (tnf, abd) in _one_process(k).items():
            tag = f"plain.k{k}.w{emit[0]}"
            assert np.array_equal(np.concatenate([p[f"{tag}.tnf"] for p in parts]), tnf), tag
            assert np.array_equal(np.concatenate([p[f"{tag}.abd"] for p in parts]), abd), tag


@pytest.mark.parametrize("world", WORLDS)
def test_quality_masked_on_several_ranks(tmp_path, world):
    """the masked plan, count half and owner merge on the masked corpus, every k: the table is the oracle's of the table text (no
    count of 0, no entry for a key nobody counted), every row ``abd_row(strict text, that table)``"""
    _run(tmp_path, world, ["qual"], KS)


def test_soft_and_quality_masked_on_two_ranks(tmp_path):
    """``lowercase_is_base``: soft-masked bases count in the table and reset the rows; a low-quality one is a base of neither plane"""
    _run(tmp_path, 2, ["soft"], KS)


def test_one_rank_plain_one_masked(tmp_path):
    """rank 1's shard has no quality plane: its count half takes the plain form, and every owner still merges with
    pg_mini_merge_bins_masked, which also takes plain parts"""
    _run(tmp_path, 2, ["mixed"], THREE_KS)


def test_counted_in_pieces_of_256_words(tmp_path):
    """PANGAEA_MINI_PIECE_WORDS=256: pg_mini_count_half_piece(_masked) and pg_mini_lookup_half_piece, some ten pieces per rank with
    reads across every seam -- the table and the rows of one piece (the workers compare), which are the oracle's"""
    _run(tmp_path, 2, ["plain", "qual"], THREE_KS, pieces=True)
