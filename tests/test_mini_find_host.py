"""pg_mini_find_applies / pg_mini_find (abundance rows against a finished mini table: what `count_kmer -g DUMP` computes,
cpptools/count_kmer.cpp:55-108,87) as far as the host decides about them: declared, exported, the applies rule, and every refusal
returned BEFORE anything is enqueued -- the descriptors and buffers carry fake addresses that are never dereferenced.  No kernel is
launched."""
import ctypes as C
import os
import re

import pytest

from pangaea_amd import _lib

from .conftest import ROOT

OK, EINVAL = 0, -1
FAKE = 0x7F0000000000            # 256-byte aligned addresses that belong to nobody, 2^36 bytes apart
A1, A2, A3, A4, A5, A6, A7 = (FAKE + (i << 36) for i in range(1, 8))
SAT = _lib.HASH_COUNT_SAT


def _table(kind=_lib.TABLE_MINI, k=21, log2_slots=20, log2_bucket_slots=10, data=FAKE):
    return _lib.pg_table(kind, k, log2_slots, log2_bucket_slots, data)


def _ref(t):
    return None if t is None else C.byref(t)


def test_header_declares_and_library_exports_the_two_entries():
    hdr = open(os.path.join(ROOT, "include", "pangaea_feat.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+9\b", hdr)                       # additive: the version stays
    assert _lib.ABI_VERSION == 9 and _lib.load().pg_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+pg_mini_find_applies\s*\(\s*const pg_table \*t,\s*int64_t n_rows,\s*int window,\s*int vsize\s*\)", code)
    assert re.search(r"int\s+pg_mini_find\s*\(\s*const uint64_t \*codes,\s*const uint32_t \*valid,\s*int64_t word_begin,\s*int64_t word_end,\s*const pg_table \*t,"
                     r"\s*const pg_rows \*rows,\s*void \*plan_ws,\s*int64_t plan_ws_bytes,\s*void \*rec_ws,\s*int64_t rec_ws_bytes,"
                     r"\s*int window,\s*int vsize,\s*void \*shuffle_ws,\s*int64_t shuffle_ws_bytes,\s*void \*merge_ws,\s*int64_t merge_ws_words,"
                     r"\s*uint32_t \*status,\s*void \*stream\s*\)", code)
    # the comment in front of them cites what they replace
    doc = hdr[:hdr.index("int pg_mini_find_applies(")].rsplit("/*", 1)[1]
    assert "count_kmer.cpp:55-108" in doc and "count_kmer.cpp:87" in doc and "pg_mini_find_applies" in doc and "pg_mini_find " in doc
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name in ("pg_mini_find_applies", "pg_mini_find"):
        assert hasattr(raw, name) and name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int
    assert len(L.pg_mini_find_applies.argtypes) == 4
    # the same arguments as pg_mini_count
    assert len(L.pg_mini_find.argtypes) == 18 and list(L.pg_mini_find.argtypes) == list(L.pg_mini_count.argtypes)


@pytest.mark.parametrize("t,n_rows,window,vsize,want", [
    (_table(), 1000, 10, 400, 1),
    (_table(), 1, 1, 1, 1),
    (_table(k=13, log2_slots=18, log2_bucket_slots=12), 50_000, 10, 400, 1),
    (_table(k=15, log2_slots=14, log2_bucket_slots=14), 3, 1, 6, 1),                # one bucket
    (_table(log2_slots=29, log2_bucket_slots=13), 100_000, 10, 400, 1),             # 2^16 buckets
    # window x vsize: the exact range of the packed counts
    (_table(), 1000, SAT // 512, 512, 1),
    (_table(), 1000, SAT // 512 + 1, 512, 0),
    (_table(), 1000, SAT, 1, 1),
    (_table(), 1000, SAT + 1, 1, 0),
    (_table(), 1000, 10, 513, 0),                                                   # beyond PG_SHUFFLE_MAX_VSIZE
    (_table(), 1000, 0, 400, 0),
    (_table(), 1000, 10, 0, 0),
    (_table(), 1000, -1, 400, 0),
    # rows: the merged lookups' rule (pg_mini_merge_form_applies)
    (_table(), 0, 10, 400, 0),
    (_table(), 1 << 19, 10, 400, 1),                                                # 13 row-group bits + 6 + 9 bin bits = 28
    (_table(), (1 << 19) + 1, 10, 400, 0),                                          # 14 row-group bits: 29
    (_table(), (1 << 20) - 1, 10, 2, 1),                                            # fewer than 2^20 rows
    (_table(), 1 << 20, 10, 2, 0),
    (_table(log2_slots=24, log2_bucket_slots=14), (1 << 18) - 2, 1, 2, 1),          # fewer than 2^(32 - 14) - 1 rows: the slot form
    (_table(log2_slots=24, log2_bucket_slots=14), (1 << 18) - 1, 1, 2, 0),
    # kinds
    (_table(_lib.TABLE_MINI_WIDE, 25, 20, 13), 1000, 10, 400, 0),
    (_table(_lib.TABLE_MINI_WIDE, 31, 20, 13), 1000, 10, 400, 0),
])
def test_find_applies(t, n_rows, window, vsize, want):
    L = _lib.load()
    assert L.pg_mini_find_applies(_ref(t), n_rows, window, vsize) == want
    if want == 1:
        assert L.pg_mini_merge_form_applies(_ref(t), n_rows, vsize) == 1


@pytest.mark.parametrize("t,n_rows,text", [
    (None, 10, "table descriptor is null"),
    (_table(data=None), 10, "table descriptor is null"),
    (_table(_lib.TABLE_HASH), 10, "needs a PG_TABLE_MINI or PG_TABLE_MINI_WIDE table"),
    (_table(_lib.TABLE_DENSE, 8), 10, "needs a PG_TABLE_MINI or PG_TABLE_MINI_WIDE table"),
    (_table(k=12), 10, "mini tables need 13 <= k <= 21 (got 12)"),
    (_table(k=22), 10, "mini tables need 13 <= k <= 21 (got 22)"),
    (_table(log2_bucket_slots=15), 10, "log2_bucket_slots 15 out of range"),
    (_table(log2_slots=31, log2_bucket_slots=14), 10, "2^17 buckets"),
    (_table(), -1, "negative row count"),
])
def test_find_applies_bad_descriptor(t, n_rows, text):
    L = _lib.load()
    assert L.pg_mini_find_applies(_ref(t), n_rows, 10, 400) == EINVAL
    msg = L.pg_last_error().decode()
    assert msg.startswith("pg_mini_find_applies: ") and text in msg


def _sizes(t, n_words, n_rows, vsize, n_records):
    L = _lib.load()
    return dict(plan=L.pg_mini_plan_bytes(n_words, _ref(t)), rec=L.pg_mini_records_bytes(n_records, _ref(t)),
                shuffle=L.pg_mini_shuffle_bytes_merged(n_words, n_rows, vsize, _ref(t)),
                merge=L.pg_mini_merge_words(n_words, n_records, n_records, _ref(t)))


N_WORDS, N_ROWS, N_RECORDS = 4096, 100, 40_000


def _find(t=None, codes=A1, valid=A2, w0=0, w1=N_WORDS, rows="ok", plan=A3, plan_bytes=None, rec=A4, rec_bytes=None, window=10, vsize=400,
          shuffle=A5, shuffle_bytes=None, merge=A6, merge_words=None, status=A7):
    L = _lib.load()
    t = _table() if t is None else t
    sz = _sizes(t, N_WORDS, N_ROWS, 400, N_RECORDS)
    if min(sz.values()) <= 0:                                    # (a table the sizing entries refuse too: sizes of the default one)
        sz = _sizes(_table(), N_WORDS, N_ROWS, 400, N_RECORDS)
    r = _lib.pg_rows(A1 + 4096, A1 + 8192, N_ROWS) if rows == "ok" else rows
    rc = L.pg_mini_find(codes, valid, w0, w1, _ref(t), _ref(r),
                        plan, sz["plan"] if plan_bytes is None else plan_bytes, rec, sz["rec"] if rec_bytes is None else rec_bytes,
                        window, vsize, shuffle, sz["shuffle"] if shuffle_bytes is None else shuffle_bytes,
                        merge, sz["merge"] if merge_words is None else merge_words, status, None)
    return rc, L.pg_last_error().decode()


@pytest.mark.parametrize("kw,text", [
    # rows are required
    (dict(rows=None), "pg_mini_find: needs rows"),
    (dict(rows=_lib.pg_rows(A1 + 4096, A1 + 8192, 0)), "pg_mini_find: needs rows"),
    (dict(rows=_lib.pg_rows(None, A1 + 8192, N_ROWS)), "pg_mini_find: null row arrays"),
    (dict(rows=_lib.pg_rows(A1 + 4096, A1 + 8192, (1 << 20) - 1)), "rows (at most"),
    # the table: a descriptor, a packed mini table
    (dict(t=_table(data=None)), "pg_mini_find: table descriptor is null"),
    (dict(t=_table(_lib.TABLE_HASH)), "pg_mini_find: needs a PG_TABLE_MINI or PG_TABLE_MINI_WIDE table"),
    (dict(t=_table(_lib.TABLE_DENSE, 8)), "pg_mini_find: needs a PG_TABLE_MINI or PG_TABLE_MINI_WIDE table"),
    (dict(t=_table(_lib.TABLE_WIDE, 25, 20, 0)), "pg_mini_find: needs a PG_TABLE_MINI or PG_TABLE_MINI_WIDE table"),
    (dict(t=_table(_lib.TABLE_MINI_WIDE, 25, 20, 13)), "pg_mini_find: packed mini tables (13 <= k <= 21)"),
    (dict(t=_table(k=12)), "mini tables need 13 <= k <= 21 (got 12)"),
    # the applies rule
    (dict(window=0), "pg_mini_find: does not apply"),
    (dict(vsize=0), "pg_mini_find: does not apply"),
    (dict(vsize=513), "pg_mini_find: does not apply"),
    (dict(window=SAT // 400 + 1), "pg_mini_find: does not apply to 100 rows, window 5243, vector size 400 (pg_mini_find_applies)"),
    # null arguments
    (dict(codes=None), "pg_mini_find: null argument"),
    (dict(valid=None), "pg_mini_find: null argument"),
    (dict(plan=None), "pg_mini_find: null argument"),
    (dict(rec=None), "pg_mini_find: null argument"),
    (dict(status=None), "pg_mini_find: null argument"),
    (dict(shuffle=None), "pg_mini_find: needs the shuffle workspace and the slot buffer"),
    (dict(merge=None), "pg_mini_find: needs the shuffle workspace and the slot buffer"),
    (dict(merge_words=0), "pg_mini_find: needs the shuffle workspace and the slot buffer"),
    (dict(w0=-1), "pg_mini_find: bad word range"),
    (dict(w0=10, w1=9), "pg_mini_find: bad word range"),
    # workspaces too short or misaligned
    (dict(plan_bytes=4096), "pg_mini_find: plan workspace of 4096 bytes"),
    (dict(plan=A3 + 8), "pg_mini_find: workspaces must be 256-byte aligned"),
    (dict(rec_bytes=24 * 255), "pg_mini_find: record workspace of 6120 bytes (pg_mini_records_bytes)"),
    (dict(rec=A4 + 128), "pg_mini_find: workspaces must be 256-byte aligned"),
    (dict(shuffle_bytes=1024), "pg_mini_find: shuffle workspace of 1024 bytes (256-byte aligned)"),
    (dict(shuffle=A5 + 64), "pg_mini_find: shuffle workspace of"),
    (dict(merge=A6 + 4), "pg_mini_find: workspaces must be 256-byte aligned"),
])
def test_find_refusals_come_before_any_launch(kw, text):
    rc, msg = _find(**kw)
    assert rc == EINVAL and text in msg, msg


def test_the_count_entry_keeps_its_messages():
    """pg_mini_find shares its argument checks with pg_mini_count; that entry still answers under its own name"""
    L = _lib.load()
    t = _table()
    sz = _sizes(t, N_WORDS, N_ROWS, 400, N_RECORDS)
    r = _lib.pg_rows(A1 + 4096, A1 + 8192, N_ROWS)
    rc = L.pg_mini_count(A1, A2, 0, N_WORDS, _ref(t), _ref(r), A3, 4096, A4, sz["rec"], 10, 400, A5, sz["shuffle"], A6, sz["merge"], A7, None)
    assert rc == EINVAL and L.pg_last_error().decode().startswith("pg_mini_count: plan workspace of 4096 bytes")
    rc = L.pg_mini_count(None, A2, 0, N_WORDS, _ref(t), _ref(r), A3, sz["plan"], A4, sz["rec"], 10, 400, A5, sz["shuffle"], A6, sz["merge"], A7, None)
    assert rc == EINVAL and L.pg_last_error().decode() == "pg_mini_count: null argument"
