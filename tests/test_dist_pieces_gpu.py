"""The N-rank super-k-mer form (``dist.MiniSharded``) counting a rank's share in PIECES (include/pangaea_feat.h:
pg_mini_count_half_piece / pg_mini_lookup_half_piece) and with more than 2^17 rows per rank: ranks share cuda:0 over gloo (or form
a one-rank RCCL group); rows, owners' tables and spot rows are compared with the one-process pipeline and the oracle."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import oracle
from pangaea_amd import dist as pdist
from pangaea_amd import feature, kmer, synth
from pangaea_amd.reads import ReadStream

PIECE_WORDS = 24_576          # (the 24 000-pair stream: about 113 k words per rank at 2 ranks, 75 k at 3 -- at least 3 pieces each)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _small_cfg():
    return synth.SynthConfig(n_pairs=24_000, n_barcodes=150, n_genomes=3, genome_len=40_000, fragment=10_000, sub_rate=0.01, n_rate=0.05, seed=321)


def _many_rows_cfg():
    # one pair per barcode: about 157 k rows per rank at 2 ranks (min_len 200 < the 302 characters of a run)
    return synth.SynthConfig(n_pairs=320_000, n_barcodes=320_000, n_genomes=3, genome_len=200_000, fragment=10_000, sub_rate=0.01, seed=77)


def _saturating_stream():
    # 3.1 M copies of one 21-mer in one run (about 97 k words: pieces of 24 k words cut it four times), a tandem repeat, random text
    rng = np.random.RandomState(3)
    rnd = bytes(rng.choice(list(b"ACGT"), size=60_000).astype(np.uint8))
    return ReadStream.from_runs([("a", b"A" * 1_600_000 + b"N" + b"T" * 1_500_040 + b"N"), ("b", b"ACG" * 30_000 + b"N"), ("c", rnd + b"N")],
                                device="cuda:0")


def _stream(case):
    if case == "saturate":
        return _saturating_stream(), 0
    if case == "rows":
        return synth.generate(_many_rows_cfg(), device="cuda:0"), 200
    return synth.generate(_small_cfg(), device="cuda:0"), 2000


def _worker(rank, world, port, outdir, case, backend, piece_words, shrink, k=21, window=10, vsize=400):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if piece_words:
        os.environ["PANGAEA_MINI_PIECE_WORDS"] = str(piece_words)
    else:
        os.environ.pop("PANGAEA_MINI_PIECE_WORDS", None)
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        s, min_len = _stream(case)
        part = s if case == "saturate" else pdist.shard_stream(ReadStream(s.codes.cpu(), s.valid.cpu(), s.n_chars, s.run_off, s.run_names),
                                                                rank, world).to("cuda:0")
        rows = part.rows(min_len)
        plan = kmer.Plan(rows, "cuda:0")
        applies = feature._sharded_mini_applies(part, plan, k, window, vsize, True)
        first_lb = None
        if shrink:
            # a local bucket two steps too small: the first count runs full, features_sharded_mini grows the geometry and counts again
            real = pdist.MiniSharded.geometry

            def small(*a, **kw):
                nonlocal first_lb
                log2_u, lb_u, lb_l = real(*a, **kw)
                first_lb = max(4, lb_l - 2)
                return log2_u, lb_u, first_lb
            pdist.MiniSharded.geometry = staticmethod(small)
        tnf, abd, ms = pdist.features_sharded_mini(part, plan, k, 4, window, vsize)
        assert isinstance(ms, pdist.MiniSharded) and ms.local.k == k, "the key-partitioned fallback was taken"
        if shrink:
            assert ms.local.log2_bucket > first_lb, "no regrow happened"
        pieces = ms.pieces
        c, n = ms.owned_items()
        same = again = True
        if case != "saturate":
            # counting again with the same object gives the same rows
            ms.count(part, plan)
            _, abd2 = kmer.features(part, plan, k_tnf=None, table=ms.local, window=window, vsize=vsize)
            same = bool(torch.equal(abd2, abd))
            # a part size too small for this batch: nothing is exchanged, count() exchanges again (no recount with pieces)
            ms._cap1 = 8
            ms.count(part, plan)
            _, abd3 = kmer.features(part, plan, k_tnf=None, table=ms.local, window=window, vsize=vsize)
            again = bool(torch.equal(abd3, abd))
        np.savez(os.path.join(outdir, f"p{rank}.npz"), c=c, n=n, tnf=tnf.cpu().numpy(), abd=abd.cpu().numpy(), names=np.array(rows.names),
                 pieces=pieces, applies=applies, n_rows=len(rows), same=same, again=again)
    finally:
        dist.destroy_process_group()


def _run(tmp_path, world, case="small", backend="gloo", piece_words=PIECE_WORDS, shrink=False, k=21, window=10, vsize=400):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), case, backend, piece_words, shrink, k, window, vsize), nprocs=world, join=True)
    return [np.load(str(tmp_path / f"p{r}.npz")) for r in range(world)]


def _check(parts, world, case="small", min_pieces=3, table=True, k=21, window=10, vsize=400, every_row=False):
    s, min_len = _stream(case)
    text = s.decode()
    for p in parts:
        assert int(p["pieces"]) >= min_pieces, int(p["pieces"])
        assert bool(p["same"]) and bool(p["again"])
    if case == "saturate":
        otab = oracle.Table(k, threads=4)
        for _ in range(world):
            otab.count(text)                                 # every rank holds a copy of the same reads
    else:
        otab = oracle.Table(k, threads=4).count(text)
    if table:
        codes = np.concatenate([p["c"] for p in parts]); counts = np.concatenate([p["n"] for p in parts])
        order = np.argsort(codes)
        ocodes, ocounts = otab.items()
        assert np.array_equal(codes[order], ocodes) and np.array_equal(counts[order], np.minimum(ocounts, 1 << 21))
    rows = s.rows(min_len)
    if case == "saturate":
        codes = np.concatenate([p["c"] for p in parts]); counts = np.concatenate([p["n"] for p in parts])
        assert counts.max() == 1 << 21 and (codes >> np.uint64(42)).max() == 0          # the sum stayed at 2^21, nothing carried into the code
        for p in parts:
            for r in range(len(rows)):
                assert np.array_equal(p["abd"][r], oracle.abd_row(text[rows.start[r]:rows.end[r]], k, otab, window, vsize))
        return
    names = [x for p in parts for x in p["names"].tolist()]
    assert names == list(rows.names)
    abd = np.concatenate([p["abd"] for p in parts]); tnf = np.concatenate([p["tnf"] for p in parts])
    plan = kmer.Plan(rows, "cuda:0")
    one = kmer.count_kmers(s, k, rows=plan, emit=(window, vsize))
    want_tnf, want_abd = kmer.features(s, plan, k_tnf=4, table=one, window=window, vsize=vsize)
    assert np.array_equal(abd, want_abd.cpu().numpy()) and np.array_equal(tnf, want_tnf.cpu().numpy())
    for r in range(0, len(rows), 1 if every_row else max(1, len(rows) // 16)):
        assert np.array_equal(abd[r], oracle.abd_row(text[rows.start[r]:rows.end[r]], k, otab, window, vsize))


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_pieces_on_several_ranks(tmp_path, world):
    """every rank counts its share in at least 3 pieces into its local table, the last piece leaves the entries of one count half:
    rows == the one-process rows == the oracle's, the owners' slices together == the oracle's table, counting again and an
    exchange redone after PG_STATUS_OVERFLOW_LIST give the same rows"""
    _check(_run(tmp_path, world), world)


@pytest.mark.gpu
@pytest.mark.parametrize("k,window,vsize", [(14, 3, 64), (15, 10, 400), (16, 25, 512), (17, 2, 50), (19, 1, 6)])
def test_pieces_at_other_k(tmp_path, k, window, vsize):
    """the small case on two ranks away from k = 21: the pieces' count halves and the <PIECE> lookup half in the instantiations for
    4, 6 and 8 k-mers per record, with minimizers of 11 (k <= 15) and of 13; every row against the oracle"""
    _check(_run(tmp_path, 2, k=k, window=window, vsize=vsize), 2, k=k, window=window, vsize=vsize, every_row=True)


@pytest.mark.gpu
def test_share_counted_piecewise_with_one_lookup_workgroup_per_cu(tmp_path, monkeypatch):
    """PG_LOOKUP_HALF_1024=1: the lookups of every piece in 1024-thread workgroups (what local buckets of 2^14 slots run)"""
    monkeypatch.setenv("PG_LOOKUP_HALF_1024", "1")
    _check(_run(tmp_path, 2), 2)


@pytest.mark.gpu
@pytest.mark.parametrize("piece_words", [0, 65_536])
def test_more_than_2_17_rows_per_rank(tmp_path, piece_words):
    """about 157 k rows per rank (the row shuffle takes two scatter passes) stay in the super-k-mer form, in one piece and in pieces"""
    parts = _run(tmp_path, 2, case="rows", piece_words=piece_words)
    for p in parts:
        assert int(p["n_rows"]) > 131_072 and bool(p["applies"])
    _check(parts, 2, case="rows", min_pieces=2 if piece_words else 1, table=False)


@pytest.mark.gpu
def test_pieces_saturate_across_pieces_and_ranks(tmp_path):
    _check(_run(tmp_path, 2, case="saturate"), 2, case="saturate")


@pytest.mark.gpu
def test_pieces_regrow_after_a_full_table(tmp_path):
    _check(_run(tmp_path, 2, shrink=True), 2)


@pytest.mark.gpu
def test_pieces_over_a_one_rank_rccl_group(tmp_path):
    _check(_run(tmp_path, 1, backend="nccl"), 1)


@pytest.mark.gpu
def test_pieces_through_the_checked_build():
    """the pieces' kernels with every global store checked against its buffer (PANGAEA_LIB=checked: PG_STATUS_BOUNDS is raised
    by MiniSharded on every rank): 2 ranks in pieces, more than 2^17 rows per rank, the one-rank RCCL group"""
    import subprocess
    import sys
    from .conftest import ROOT
    env = dict(os.environ, PANGAEA_LIB="checked")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_dist_pieces_gpu.py"),
                        "-k", "(pieces_on_several_ranks and 2) or more_than_2_17_rows or one_rank_rccl or at_other_k"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "no tests ran" not in r.stdout
