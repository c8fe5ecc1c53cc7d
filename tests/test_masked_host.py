"""CPU checks of the masked N-rank super-k-mer form: the exports, the union plane of a ReadStream, the dispatch rules."""
import numpy as np
import torch

from pangaea_amd import _lib
from pangaea_amd import dist as pdist
from pangaea_amd.kmer import KmerTable
from pangaea_amd.reads import ReadStream


def _stream(lower=None, lowq=None):
    valid = torch.tensor([0x0FFF_FFFF, 0x7FFF_FFF0], dtype=torch.int32)
    return ReadStream(torch.zeros(2, dtype=torch.int64), valid, 64, np.array([0, 64], dtype=np.int64), ["a"],
                      valid_lower=None if lower is None else torch.tensor(lower, dtype=torch.int32),
                      valid_lowq=None if lowq is None else torch.tensor(lowq, dtype=torch.int32))


def test_masked_entries_are_exported():
    L = _lib.load()
    for name in ("pg_mini_plan_masked", "pg_mini_count_half_masked", "pg_mini_count_half_piece_masked", "pg_mini_merge_bins_masked"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert _lib.ABI_VERSION == 9 and L.pg_abi_version() == 9


def test_union_plane():
    plain = _stream()
    assert plain.union_valid(True) is plain.valid and not KmerTable.half_masked(plain, True)
    soft = _stream(lower=[0x3000_0000, 0x0000_000F])
    assert soft.union_valid(True) is soft.table_valid(True) and KmerTable.half_masked(soft, True)
    assert soft.union_valid(False) is soft.valid and not KmerTable.half_masked(soft, False)
    qual = _stream(lowq=[0x0000_0010, 0x0000_0100])
    assert qual.union_valid(False) is qual.valid and qual.union_valid(True) is qual.valid
    assert KmerTable.half_masked(qual, False) and KmerTable.half_masked(qual, True)
    both = _stream(lower=[0x3000_0000, 0x0000_000F], lowq=[0x1000_0010, 0x0000_0100])
    u = both.union_valid(True)
    assert torch.equal(u, both.table_valid(True) | both.valid) and both.union_valid(True) is u       # cached
    # (a low-quality upper-case base stays valid for the rows; a low-quality lower-case one is valid for neither)
    assert torch.equal(u, both.valid | (both.valid_lower & ~both.valid_lowq))


def test_masked_rows_rule(monkeypatch):
    assert pdist.MiniSharded.masked_rows_apply(21, 1000, 400) and pdist.MiniSharded.masked_rows_apply(15, 1000, 6)
    assert pdist.MiniSharded.masked_rows_apply(21, 300_000, 400)
    assert not pdist.MiniSharded.masked_rows_apply(21, _lib.MINI_MASKED_MAX_ROWS + 1, 6)
    assert not pdist.MiniSharded.masked_rows_apply(21, 0, 400)
    monkeypatch.setenv("PG_MINI_MERGE", "0")
    assert not pdist.MiniSharded.masked_rows_apply(21, 1000, 400)


def test_poly_a_generator_follows_k():
    """the poly-A streams of test_dist_masked_gpu.py at k = 15 and k = 21: every row holds all-A k-mer windows in the strict text,
    none of them is in the table's text of "polya0" (each is cut by a low-quality base: row-only), "polya" is the same text with
    clean A runs behind the first six rows -- and a generator made for another k would not do (its clean stretches reach k, or its
    runs do not).  The k = 21 stream is the one the tests have always run: 30, 30 and 25 with marks at 15, 14 and 12."""
    from oracle import oracle
    from .test_dist_masked_gpu import _has_poly_a, _stream
    for k in (15, 21):
        s0, s1 = _stream("polya0", k), _stream("polya", k)
        strict, table = s0.decode(), s0.decode(plane=s0.table_valid(False))
        if k == 21:
            r0 = strict[:int(s0.run_off[1])]
            assert r0[120:150] == b"A" * 30 and r0[230:260] == b"T" * 30 and r0[320:345] == b"A" * 25
            assert [i for i in range(len(r0)) if table[i] != r0[i]] == [135, 244, 332]
        assert len(strict) == len(table) and strict != table
        off = s0.run_off
        for i in range(len(off) - 1):
            assert _has_poly_a(strict[int(off[i]):int(off[i + 1])], k)
        assert not _has_poly_a(table, k)
        assert 0 not in set(oracle.Table(k).count(table).items()[0].tolist())
        t1 = s1.decode(plane=s1.table_valid(False))
        assert 0 in set(oracle.Table(k).count(t1).items()[0].tolist())
        off1 = s1.run_off
        for i in range(len(off) - 1):                      # the marked part of every run is polya0's
            n = int(off[i + 1] - off[i]) - 1
            assert t1[int(off1[i]):int(off1[i]) + n] == table[int(off[i]):int(off[i]) + n]
            assert _has_poly_a(t1[int(off1[i]):int(off1[i + 1])], k) == (i < 6)
    # the run lengths have to follow k: the stream made for k = 21 would count the all-A 15-mer (clean stretches of 15)
    s21 = _stream("polya0", 21)
    assert _has_poly_a(s21.decode(plane=s21.table_valid(False)), 15)
