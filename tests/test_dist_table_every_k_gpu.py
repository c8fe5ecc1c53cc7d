"""The key-partitioned multi-rank path (``dist.count_kmers_sharded`` -> ``dist.exchange_table``: what N > 1 ranks run wherever the
super-k-mer form does not apply -- k < 13, k > 21, PANGAEA_NO_MINI=1) away from k = 21: the dense table's all-reduce (k <= 8), hash
tables below the minimizer pipeline's smallest k, the bucketed exchange in its 8-byte and its 6-byte format, and wide tables
(k > 21), whose exchange adds the other ranks' entries with global atomics.  Ranks share cuda:0 over gloo, as in test_dist_gloo.py;
every rank's table is compared with the oracle's table of the whole stream, the ranks' rows together with the oracle's rows."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import oracle
from pangaea_amd import _lib
from pangaea_amd import dist as pdist
from pangaea_amd import kmer, synth
from pangaea_amd.reads import ReadStream

# k -> (window, vsize) of the rows; the groups share one spawn each (the start of the processes is most of such a test's time)
_WV = {6: (100, 400), 8: (10, 400), 11: (2, 50), 12: (3, 64), 15: (10, 400), 17: (1, 6), 21: (10, 400), 22: (10, 400), 27: (1, 6), 31: (3, 700)}
_GROUPS = {"dense": (6, 8), "hash-small": (11, 12), "hash-bucketed": (15, 17, 21), "wide": (22, 27, 31)}
_FORCED = ((20, "8-byte"), (21, "6-byte"))        # with_slots sizes of the forced exchanges: 2^10 buckets (32 tag bits) and 2^11 (31)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _stream(k):
    """the stream of test_gpu_parity.py::test_synthetic_against_oracle: 3000 pairs, 37 barcodes, a fifth of the bases N"""
    cfg = synth.SynthConfig(n_pairs=3000, n_barcodes=37, n_genomes=3, genome_len=30_000, fragment=8_000, sub_rate=0.01, n_rate=0.2, seed=100 + k)
    return synth.generate(cfg, device="cuda:0")


def _low_complexity_stream():
    """the stream of test_mini_gpu.py::test_mini_low_complexity_runs_and_saturating_counts: 3.1 M copies of one k-mer"""
    rng = np.random.RandomState(11)
    rnd = bytes(rng.choice(list(b"ACGT"), size=30_000).astype(np.uint8))
    return ReadStream.from_runs([("a", b"A" * 1_600_000 + b"N" + b"T" * 1_500_040 + b"N"),
                                 ("b", b"AC" * 40_000 + b"N" + b"ACG" * 30_000 + b"N" + b"AACCGGTT" * 9_000 + b"N"),
                                 ("c", rnd + b"N" + rnd[:20_000] + b"N")], device="cuda:0")


def _shard_by_runs(s, rank, world):
    return pdist.shard_stream(ReadStream(s.codes.cpu(), s.valid.cpu(), s.n_chars, s.run_off, s.run_names), rank, world).to("cuda:0")


def _worker(rank, world, port, outdir, ks, forced):
    _init(rank, world, port)
    taken = []                     # which of the 6-byte forms _exchange_bucketed called (none: the 8-byte all-gather)
    originals = {name: getattr(pdist, name) for name in ("_exchange_planes", "_exchange_owner")}
    for name, orig in originals.items():
        setattr(pdist, name, lambda *a, _orig=orig, _name=name, **kw: (taken.append(_name), _orig(*a, **kw))[1])
    try:
        out = {}
        for k in ks:
            window, vsize = _WV[k]
            part = _shard_by_runs(_stream(k), rank, world)
            rows = part.rows(2000)
            plan = kmer.Plan(rows, "cuda:0")
            runs = [("sized", None)] + ([(f"slots{log2}", log2) for log2, _ in _FORCED] if forced and k != 21 else [])
            for tag, log2 in runs:
                del taken[:]
                if log2 is None:
                    table = pdist.count_kmers_sharded(part, k, rows=plan)
                else:                                       # a deferred count into a table of a given size, as the path makes them
                    table = kmer.KmerTable.with_slots(k, "cuda:0", log2, 10)
                    table.count(part, rows=plan, deferred_group=1)
                    assert table.pending
                    pdist.exchange_table(table)
                assert table.k == k and table.kind == kmer.KmerTable.default_kind(k) and not table.pending
                c, n = table.items()
                tnf, abd = kmer.features(part, plan, k_tnf=4, table=table, window=window, vsize=vsize)
                out.update({f"c{k}{tag}": c, f"n{k}{tag}": n, f"tnf{k}{tag}": tnf.cpu().numpy(), f"abd{k}{tag}": abd.cpu().numpy(),
                            f"names{k}{tag}": np.array(rows.names)})
                if table.kind == "hash":
                    out[f"bucketed{k}{tag}"] = table._bucketed()
                    out[f"tag_bits{k}{tag}"] = table.tag_bits if table._bucketed() else -1
                    out[f"six{k}{tag}"] = len(taken) > 0
                del table
        np.savez(os.path.join(outdir, f"t{rank}.npz"), **out)
    finally:
        for name, orig in originals.items():
            setattr(pdist, name, orig)
        dist.destroy_process_group()


_ORACLE = {}


def _oracle(k):
    """(codes, counts, names, tnf, abd) of the whole stream at k -- computed once, shared by the worlds"""
    if k not in _ORACLE:
        s = _stream(k)
        text = s.decode()
        rows = s.rows(2000)
        assert len(rows) == 37
        otab = oracle.Table(k, threads=4).count(text)
        window, vsize = _WV[k]
        segs = [text[int(a):int(b)] for a, b in zip(rows.start, rows.end)]
        _ORACLE[k] = otab.items() + (list(rows.names), np.stack([oracle.tnf_row(x, 4) for x in segs]),
                                     np.stack([oracle.abd_row(x, k, otab, window, vsize) for x in segs]))
    return _ORACLE[k]


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("group", sorted(_GROUPS))
def test_key_partitioned_tables_at_every_kind_of_k(tmp_path, group, world):
    """every rank counts its runs and exchanges: afterwards EVERY rank holds the oracle's table of the whole stream, and the ranks'
    rows in rank order are the oracle's rows -- dense (k = 6, 8), hash below the minimizer pipeline (11, 12), hash with the bucketed
    exchange (15, 17, 21; on two ranks also into tables of 2^20 and 2^21 slots: the 8-byte and the 6-byte format), wide (22, 27, 31)"""
    ks = _GROUPS[group]
    forced = group == "hash-bucketed" and world == 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), ks, forced), nprocs=world, join=True)
    parts = [np.load(str(tmp_path / f"t{r}.npz")) for r in range(world)]
    formats = set()
    for k in ks:
        ocodes, ocounts, onames, otnf, oabd = _oracle(k)
        want_counts = np.minimum(ocounts, _lib.HASH_COUNT_SAT) if 8 < k <= 21 else ocounts
        for tag, want_six in [("sized", None)] + ([(f"slots{log2}", fmt == "6-byte") for log2, fmt in _FORCED] if forced and k != 21 else []):
            for r, p in enumerate(parts):
                assert np.array_equal(p[f"c{k}{tag}"], ocodes) and np.array_equal(p[f"n{k}{tag}"], want_counts), (k, tag, r)
            assert [n for p in parts for n in p[f"names{k}{tag}"].tolist()] == onames, (k, tag)
            assert np.array_equal(np.concatenate([p[f"tnf{k}{tag}"] for p in parts]), otnf), (k, tag)
            assert np.array_equal(np.concatenate([p[f"abd{k}{tag}"] for p in parts]), oabd), (k, tag)
            if group != "hash-bucketed":
                continue
            # the exchange format: the same on every rank; 6 bytes per entry only where a tag fits 31 bits
            six, bits = {bool(p[f"six{k}{tag}"]) for p in parts}, {int(p[f"tag_bits{k}{tag}"]) for p in parts}
            assert len(six) == len(bits) == 1 and all(bool(p[f"bucketed{k}{tag}"]) for p in parts), (k, tag)
            six, bits = six.pop(), bits.pop()
            print(f"k={k} {tag}: tag_bits {bits}, {'6' if six else '8'}-byte format")
            assert not six or bits <= 31, (k, tag)
            if want_six is not None:
                assert six == want_six and (bits <= 31) == want_six, (k, tag, bits)
            if k != 21:
                formats.add(six)
    assert not forced or formats == {False, True}           # both formats ran at a k other than 21


def _wide_sat_worker(rank, world, port, outdir):
    _init(rank, world, port)
    try:
        s = _low_complexity_stream()                          # every rank holds a copy of the same reads
        table = pdist.count_kmers_sharded(s, 25, rows=kmer.Plan(s.rows(0), "cuda:0"))
        assert table.kind == "wide"
        c, n = table.items()
        np.savez(os.path.join(outdir, f"w{rank}.npz"), c=c, n=n)
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_wide_exchange_counts_past_the_packed_limit(tmp_path):
    """k = 25 on two ranks that both hold 3.1 M copies of one k-mer: the exchanged wide table is the oracle's table of the text
    counted twice, exactly -- wide counts do not stop at 2^21"""
    mp.spawn(_wide_sat_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    text = _low_complexity_stream().decode()
    otab = oracle.Table(25, threads=4)
    for _ in range(2):
        otab.count(text)
    ocodes, ocounts = otab.items()
    assert ocounts.max() > 6_000_000
    for r in range(2):
        p = np.load(str(tmp_path / f"w{r}.npz"))
        assert np.array_equal(p["c"], ocodes) and np.array_equal(p["n"], ocounts), r
        assert p["n"].max() > 6_000_000
