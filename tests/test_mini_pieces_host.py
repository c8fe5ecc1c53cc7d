"""CPU-only checks of the N-rank pieces entries (include/pangaea_feat.h: pg_mini_count_half_piece and its neighbours): they are
exported, the two host-side rules (record layout, merged-lookups predicate) agree with a restatement here, and the pure budget
function behind ``KmerTable.count_half`` chooses one piece, pieces or nothing as it should.  No kernel is launched here."""
import ctypes as C
import os

import pytest

from pangaea_amd import _lib, kmer
from pangaea_amd.dist import MiniSharded

NEW = ["pg_mini_count_half_piece", "pg_mini_lookup_half_piece", "pg_mini_merge_form_applies", "pg_mini_records_meta_offset"]


def _desc(k=21, log2_slots=25, log2_bucket=12, kind=_lib.TABLE_MINI):
    return _lib.pg_table(kind, k, log2_slots, log2_bucket, 1)     # (geometry only: the host rules never read the data pointer)


def test_new_symbols_are_exported_and_declared():
    L = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pangaea_feat.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert f"{name}(" in hdr, name
    assert _lib.load().pg_abi_version() == 9


@pytest.mark.parametrize("log2_slots,log2_bucket", [(25, 12), (30, 14), (20, 9)])
def test_records_meta_offset_is_the_fourth_plane(log2_slots, log2_bucket):
    L = _lib.load()
    t = _desc(log2_slots=log2_slots, log2_bucket=log2_bucket)
    for n_records in (0, 1, 255, 256, 4097, 123_457, 10_000_000):
        ws = L.pg_mini_records_bytes(n_records, C.byref(t))
        for extra in (0, 1, 23, 24 * 256 - 1, 24 * 256, 1 << 20):
            nbytes = ws + extra
            cap = nbytes // 24 // 256 * 256               # [bases A | bases B | meta A | meta B], cap records each
            assert L.pg_mini_records_meta_offset(nbytes, C.byref(t)) == 8 * cap + 8 * cap + 4 * cap
            assert 24 * cap <= nbytes and cap >= n_records
    assert L.pg_mini_records_meta_offset(100, C.byref(t)) < 0          # (no room for one block of 256 records)


def _merge_form(n_rows, vsize, log2_bucket):
    want = os.environ.get("PG_MINI_MERGE")
    if (want is not None and not want.strip().lstrip("-").isdigit()) or (want is not None and int(want) == 0) or os.environ.get("PG_MINI_NO_MERGE"):
        return False
    if not (0 < n_rows < (1 << (32 - log2_bucket)) - 1) or os.environ.get("PG_MINI_PROBE_TWICE"):
        return False
    if vsize < 1 or n_rows >= (1 << 20):
        return False
    vbits = max(1, (vsize - 1).bit_length())
    gbits = ((n_rows + 63) // 64 - 1).bit_length()
    return vbits + 6 + gbits <= 28


def _grid():
    rows = [1, 63, 64, 65, 131_071, 131_072, 150_000, 262_142, 262_143, 262_144, 300_000, (1 << 19) - 2, (1 << 19) - 1,
            1 << 19, (1 << 19) + 1, 600_000, (1 << 20) - 2, 1 << 20]
    for lb in (4, 9, 12, 13, 14):
        for vsize in (1, 2, 200, 256, 257, 400, 512):
            for n in rows:
                yield n, vsize, lb


def test_merge_form_applies_agrees_with_the_rule(monkeypatch):
    for var in ("PG_MINI_MERGE", "PG_MINI_NO_MERGE", "PG_MINI_PROBE_TWICE"):
        monkeypatch.delenv(var, raising=False)
    L = _lib.load()
    for n, vsize, lb in _grid():
        t = _desc(log2_slots=lb + 10, log2_bucket=lb)
        assert L.pg_mini_merge_form_applies(C.byref(t), n, vsize) == int(_merge_form(n, vsize, lb)), (n, vsize, lb)
    # the boundary the N-rank form now reaches: 2^19 rows at -v 400 (buckets of 2^13 slots), one more row does not fit
    t13 = _desc(log2_slots=23, log2_bucket=13)
    assert L.pg_mini_merge_form_applies(C.byref(t13), (1 << 19) - 2, 400) == 1
    assert L.pg_mini_merge_form_applies(C.byref(t13), (1 << 19) + 1, 400) == 0
    # wide tables never take the merged lookups; a bad table is an error
    assert L.pg_mini_merge_form_applies(C.byref(_desc(k=25, log2_slots=20, log2_bucket=12, kind=_lib.TABLE_MINI_WIDE)), 1000, 400) == 0
    assert L.pg_mini_merge_form_applies(C.byref(_desc(log2_slots=40, log2_bucket=12)), 1000, 400) < 0


def test_merge_form_applies_follows_the_environment(monkeypatch):
    L = _lib.load()
    t = _desc(log2_slots=22, log2_bucket=12)
    monkeypatch.delenv("PG_MINI_NO_MERGE", raising=False)
    monkeypatch.setenv("PG_MINI_MERGE", "0")
    for n, vsize, lb in _grid():
        assert L.pg_mini_merge_form_applies(C.byref(_desc(log2_slots=lb + 10, log2_bucket=lb)), n, vsize) == 0
    monkeypatch.setenv("PG_MINI_MERGE", "1")
    assert L.pg_mini_merge_form_applies(C.byref(t), 150_000, 400) == 1


def test_rows_past_2_17_reach_the_n_rank_form(monkeypatch):
    monkeypatch.delenv("PG_MINI_MERGE", raising=False)
    assert MiniSharded.max_local_log2_bucket(100_000) == 14
    assert MiniSharded.max_local_log2_bucket(300_000) == 13
    assert MiniSharded.rows_apply(21, 131_071, 400) and MiniSharded.rows_apply(21, 150_000, 400)
    assert MiniSharded.rows_apply(21, 250_000, 400) and MiniSharded.rows_apply(21, 500_000, 400)
    assert not MiniSharded.rows_apply(21, 600_000, 400)
    # the local bucket stays inside the slot form whatever the estimate asks for
    _, _, lb = MiniSharded.geometry(1 << 33, 1 << 31, n_rows=500_000)
    assert lb == 13
    assert MiniSharded.geometry(1 << 33, 1 << 31) == MiniSharded.geometry(1 << 33, 1 << 31, n_rows=1000)


GB = 1 << 30


def test_budget_one_piece_when_everything_fits():
    # a 10 M-pair share (~94 M words) on a free GPU, local geometry of 2^16 buckets of 2^12 slots, 8 ranks
    n = 94_500_000
    assert kmer.half_piece_words(280 * GB, n, 28, 12, 50_000, 8) == n
    assert kmer.half_piece_words(280 * GB, n, 28, 12, 250_000, 8) == n


def test_budget_pieces_when_one_piece_does_not_fit():
    n = 661_000_000                                      # ~70 M pairs
    w = kmer.half_piece_words(280 * GB, n, 29, 13, 100_000, 2)
    assert w is not None and w < n and w % _lib.WORD_ALIGN == 0
    # what the function promises: everything held with pieces of w words fits 85 % of the free bytes
    rec, slots, words = kmer.KmerTable._PIECE_BYTES_PER_WORD
    held = (slots + 28 + words + 4) * n + rec * w + (8 + 8 + 8 / 64) * (1 << 29) + 4 * (1 << 16) + 20 * (int(1.04 * (1 << 29)) + 16)
    assert held <= 0.85 * 280 * GB
    # less memory, smaller pieces
    w2 = kmer.half_piece_words(250 * GB, n, 29, 13, 100_000, 2)
    assert w2 is not None and w2 < w
    # the rows' two scatter passes cost a second word buffer: more rows, smaller pieces (or none)
    w3 = kmer.half_piece_words(280 * GB, n, 29, 13, 300_000, 2)
    assert w3 is None or w3 < w


def test_budget_none_when_not_even_pieces_fit():
    assert kmer.half_piece_words(100 * GB, 945_000_000, 29, 13, 500_000, 2) is None
    assert kmer.half_piece_words(1 * GB, 10_000_000, 28, 12, 50_000, 8) is None
