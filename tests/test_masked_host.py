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
