"""The three table-merge entries (pg_table_merge, pg_table_merge_aligned, pg_table_merge_aligned_applies: what `jellyfish merge`
gives over the tables of src/feature.py:76-94) as far as the host decides about them: declared, exported, and every refusal returned
BEFORE anything is enqueued -- the descriptors carry fake addresses that are never dereferenced -- plus the argument handling of
`kmer_table merge`.  No kernel is launched."""
import ctypes as C
import os
import re

import pytest

from pangaea_amd import _lib, cli

from .conftest import ROOT

OK, EINVAL = 0, -1
FAKE = 0x7F0000000000            # 256-byte aligned addresses that belong to nobody, 2^36 bytes apart
OTHER = 0x7F1000000000
THIRD = 0x7F2000000000
NAMES = ("pg_table_merge", "pg_table_merge_aligned", "pg_table_merge_aligned_applies")


def _table(kind=_lib.TABLE_MINI, k=21, log2_slots=20, log2_bucket_slots=10, data=FAKE):
    return _lib.pg_table(kind, k, log2_slots, log2_bucket_slots, data)


def _hash(k=21, log2_slots=20, log2_bucket_slots=10, data=FAKE):
    return _table(_lib.TABLE_HASH, k, log2_slots, log2_bucket_slots, data)


def _ref(t):
    return None if t is None else C.byref(t)


def _merge(dst, src, status=FAKE):
    L = _lib.load()
    rc = L.pg_table_merge(_ref(dst), _ref(src), status, None)
    return rc, L.pg_last_error().decode()


def _merge_aligned(dst, srcs, n=None, status=FAKE):
    L = _lib.load()
    arr = None
    if srcs is not None:
        arr = (C.POINTER(_lib.pg_table) * max(1, len(srcs)))(*[C.pointer(t) if t is not None else C.POINTER(_lib.pg_table)() for t in srcs])
    rc = L.pg_table_merge_aligned(_ref(dst), arr, len(srcs) if n is None else n, status, None)
    return rc, L.pg_last_error().decode()


def test_header_declares_and_library_exports_the_three_entries():
    hdr = open(os.path.join(ROOT, "include", "pangaea_feat.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+9\b", hdr)                       # additive: the version stays
    assert _lib.ABI_VERSION == 9 and _lib.load().pg_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+pg_table_merge\s*\(\s*const pg_table \*dst,\s*const pg_table \*src,\s*uint32_t \*status,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+pg_table_merge_aligned\s*\(\s*const pg_table \*dst,\s*const pg_table \*const \*srcs,\s*int n_srcs,\s*uint32_t \*status,"
                     r"\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+pg_table_merge_aligned_applies\s*\(\s*const pg_table \*a,\s*const pg_table \*b\s*\)", code)
    # each entry cites what it replaces
    for name in NAMES:
        assert re.search(name + r"\s+replaces[^;]*jellyfish merge[^;]*feature\.py:76-94", hdr), name
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int
    assert len(L.pg_table_merge.argtypes) == 4 and len(L.pg_table_merge_aligned.argtypes) == 5 and len(L.pg_table_merge_aligned_applies.argtypes) == 2


@pytest.mark.parametrize("dst,src,status,text", [
    (None, _table(data=OTHER), FAKE, "pg_table_merge: dst is null"),
    (_table(), None, FAKE, "pg_table_merge: src is null"),
    (_table(), _table(data=OTHER), None, "pg_table_merge: status is null"),
    (_table(data=None), _table(data=OTHER), FAKE, "table descriptor is null"),
    (_table(), _table(data=None), FAKE, "table descriptor is null"),
    (_table(k=21), _table(k=15, data=OTHER), FAKE, "pg_table_merge: k differs (dst 21, src 15)"),
    (_hash(k=11), _table(_lib.TABLE_DENSE, k=12, data=OTHER), FAKE, "pg_table_merge: k differs (dst 11, src 12)"),
    # a kind that does not admit k
    (_hash(k=25), _table(_lib.TABLE_WIDE, 25, 20, 0, OTHER), FAKE, "hash table needs 1 <= k <= 21 (got 25)"),
    (_table(_lib.TABLE_DENSE, k=21), _table(data=OTHER), FAKE, "dense table needs 1 <= k <= 16 (got 21)"),
    (_table(k=11), _hash(k=11, data=OTHER), FAKE, "mini table needs 13 <= k <= 21 (got 11)"),
    (_table(_lib.TABLE_MINI_WIDE, k=21, log2_bucket_slots=13), _table(data=OTHER), FAKE, "wide mini table needs 21 < k <= 31 (got 21)"),
    (_table(_lib.TABLE_WIDE, 25, 20, 0), _table(k=25, data=OTHER), FAKE, "mini table needs 13 <= k <= 21 (got 25)"),
    (_table(kind=9), _table(data=OTHER), FAKE, "unknown table kind 9"),
    # the destination may not be, or overlap, the source
    (_table(), _table(), FAKE, "pg_table_merge: dst aliases src"),
    (_table(), _hash(data=FAKE + (4 << 20)), FAKE, "pg_table_merge: dst aliases src"),
    (_hash(log2_slots=12, log2_bucket_slots=0, data=FAKE + 4096), _table(_lib.TABLE_WIDE, 21, 20, 0, FAKE), FAKE, "pg_table_merge: dst aliases src"),
    (_table(), _table(data=OTHER + 8), FAKE, "pg_table_merge: t->data is not 16-byte aligned"),
])
def test_merge_refusals(dst, src, status, text):
    rc, msg = _merge(dst, src, status)
    assert rc == EINVAL and msg == text


@pytest.mark.parametrize("dst,srcs,n,status,text", [
    (None, [_table(data=OTHER)], None, FAKE, "pg_table_merge_aligned: dst is null"),
    (_table(), None, 1, FAKE, "pg_table_merge_aligned: srcs is null"),
    (_table(), [_table(data=OTHER)], None, None, "pg_table_merge_aligned: status is null"),
    (_table(), [_table(data=OTHER)], 0, FAKE, "pg_table_merge_aligned: n_srcs 0 outside [1, 16]"),
    (_table(), [_table(data=OTHER)], -1, FAKE, "pg_table_merge_aligned: n_srcs -1 outside [1, 16]"),
    (_table(), [_table(data=OTHER)] * 17, None, FAKE, "pg_table_merge_aligned: n_srcs 17 outside [1, 16]"),
    (_table(), [_table(data=OTHER), None], None, FAKE, "pg_table_merge_aligned: srcs[1] is null"),
    (_table(), [_table(data=OTHER), _table(k=15, data=THIRD)], None, FAKE, "pg_table_merge_aligned: k differs (dst 21, srcs[1] 15)"),
    (_table(k=22), [_table(data=OTHER)], None, FAKE, "mini table needs 13 <= k <= 21 (got 22)"),
    (_table(), [_hash(k=22, data=OTHER)], None, FAKE, "hash table needs 1 <= k <= 21 (got 22)"),
    # differing geometry, differing kinds, kinds the aligned form does not take
    (_table(), [_table(log2_slots=21, data=OTHER)], None, FAKE, "of one geometry"),
    (_table(), [_table(data=OTHER), _table(log2_bucket_slots=11, data=THIRD)], None, FAKE, "dst and srcs[1] are not mini tables, or bucketed hash tables, of one geometry"),
    (_table(), [_hash(data=OTHER)], None, FAKE, "of one geometry"),
    (_hash(log2_bucket_slots=0), [_hash(log2_bucket_slots=0, data=OTHER)], None, FAKE, "of one geometry"),
    (_table(_lib.TABLE_WIDE, 25, 20, 0), [_table(_lib.TABLE_WIDE, 25, 20, 0, OTHER)], None, FAKE, "of one geometry"),
    (_table(_lib.TABLE_DENSE, 8), [_table(_lib.TABLE_DENSE, 8, data=OTHER)], None, FAKE, "of one geometry"),
    # the destination may not be, or overlap, a source (the same source twice is fine: see the GPU tests)
    (_table(), [_table(data=OTHER), _table()], None, FAKE, "pg_table_merge_aligned: dst aliases srcs[1]"),
    (_table(), [_table(data=FAKE + (1 << 20))], None, FAKE, "pg_table_merge_aligned: dst aliases srcs[0]"),
    (_table(data=FAKE + 8), [_table(data=OTHER)], None, FAKE, "pg_table_merge_aligned: dst->data is not 16-byte aligned"),
    (_table(), [_table(data=OTHER + 8)], None, FAKE, "pg_table_merge_aligned: srcs[0]->data is not 16-byte aligned"),
])
def test_merge_aligned_refusals(dst, srcs, n, status, text):
    rc, msg = _merge_aligned(dst, srcs, n, status)
    assert rc == EINVAL and text in msg and (msg == text or "of one geometry" in text)


@pytest.mark.parametrize("a,b,want", [
    (_table(), _table(data=OTHER), 1),
    (_table(), _table(), 1),                                                   # (geometry only: the data is not looked at)
    (_table(k=13, log2_slots=18, log2_bucket_slots=12), _table(k=13, log2_slots=18, log2_bucket_slots=12), 1),
    (_table(log2_slots=14, log2_bucket_slots=14), _table(log2_slots=14, log2_bucket_slots=14), 1),      # one bucket, 128 KiB of LDS
    (_table(log2_slots=30, log2_bucket_slots=14), _table(log2_slots=30, log2_bucket_slots=14), 1),
    (_hash(), _hash(), 1),
    (_hash(k=11, log2_slots=24, log2_bucket_slots=14), _hash(k=11, log2_slots=24, log2_bucket_slots=14), 1),
    (_table(), _table(k=15), 0),
    (_table(), _table(log2_slots=21), 0),
    (_table(), _table(log2_bucket_slots=11), 0),
    (_table(), _hash(), 0),
    (_hash(), _table(), 0),
    (_hash(log2_bucket_slots=0), _hash(log2_bucket_slots=0), 0),                # unbucketed
    (_hash(log2_slots=20, log2_bucket_slots=15), _hash(log2_slots=20, log2_bucket_slots=15), 0),        # buckets beyond LDS
    (_hash(k=22), _hash(k=22), 0),
    (_table(k=12), _table(k=12), 0),
    (_table(log2_slots=31, log2_bucket_slots=14), _table(log2_slots=31, log2_bucket_slots=14), 0),      # more than 2^16 buckets
    (_table(_lib.TABLE_DENSE, 8), _table(_lib.TABLE_DENSE, 8), 0),
    (_table(_lib.TABLE_WIDE, 25, 20, 0), _table(_lib.TABLE_WIDE, 25, 20, 0), 0),
    (_table(_lib.TABLE_MINI_WIDE, 25, 20, 13), _table(_lib.TABLE_MINI_WIDE, 25, 20, 13), 0),
    (_table(kind=9), _table(kind=9), 0),
    (None, _table(), 0),
    (_table(), None, 0),
])
def test_merge_aligned_applies(a, b, want):
    assert _lib.load().pg_table_merge_aligned_applies(_ref(a), _ref(b)) == want


def _main(argv):
    try:
        return cli.main_kmer_table(argv)
    except SystemExit as e:
        return e.code


@pytest.mark.parametrize("argv,text", [
    (["merge", "-k", "21", "-g", "never_opened.dump", "-o", "unused.dump"], "two inputs or more"),
    (["merge", "-k", "21", "-i", "never_opened.fq", "-o", "unused.dump"], "two inputs or more"),
    (["merge", "-k", "21", "-o", "unused.dump"], "two inputs or more"),
    (["merge", "-k", "0", "-g", "never_opened.dump", "-g", "nor_this.dump", "-o", "unused.dump"], "k-mer size 0 unsupported"),
    (["merge", "-k", "32", "-g", "never_opened.dump", "-i", "nor_this.fq", "-o", "unused.dump"], "k-mer size 32 unsupported"),
    (["merge", "-k", "21", "-g", "never_opened.dump", "-g", "nor_this.dump", "-L", "0", "-o", "unused.dump"], "-L must be at least 1"),
    (["merge", "-g", "never_opened.dump", "-g", "nor_this.dump", "-o", "unused.dump"], "-k"),                 # no k at all
    (["merge", "-k", "21", "-g", "never_opened.dump", "-g", "nor_this.dump"], "-o"),                           # no output
])
def test_kmer_table_merge_bad_arguments_exit_1(argv, text, capsys, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    assert _main(argv) == 1
    out = capsys.readouterr()
    assert out.out == "" and "kmer_table" in out.err and text in out.err and "Traceback" not in out.err
    assert not os.listdir(tmp_path)
