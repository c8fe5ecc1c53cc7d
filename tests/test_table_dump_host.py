"""The dump entries (pg_table_dump_units / _sizes / _text: `jellyfish dump -c -t` of src/feature.py:87,103; pg_dump_parse: the
reload of count_kmer.cpp:139-170) as far as the host decides about them: declared with their citations, exported, and every
refusal returned BEFORE the first HIP call -- the descriptors carry fake addresses that are never dereferenced -- plus the
argument handling of `kmer_table dump`.  No kernel is launched."""
import ctypes as C
import os
import re

import pytest

from pangaea_amd import _lib, cli, kmer

from .conftest import ROOT

OK, EINVAL = 0, -1
FAKE = 0x7F0000000000            # a 256-byte aligned address that belongs to nobody
NEW = ("pg_table_dump_units", "pg_table_dump_sizes", "pg_table_dump_text", "pg_dump_parse_workspace_bytes", "pg_dump_parse")


def _table(kind=_lib.TABLE_MINI, k=21, log2_slots=20, log2_bucket_slots=10, data=FAKE):
    return _lib.pg_table(kind, k, log2_slots, log2_bucket_slots, data)


def _call(name, *args):
    L = _lib.load()
    rc = getattr(L, name)(*args)
    return rc, L.pg_last_error().decode()


def _ref(t):
    return None if t is None else C.byref(t)


def test_header_declares_and_library_exports_the_dump_entries():
    hdr = open(os.path.join(ROOT, "include", "pangaea_feat.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+9\b", hdr)                       # additive: the version stays
    m = re.search(r"#define\s+PG_DUMP_UNIT_SLOTS\s+(\d+)\b", hdr)
    unit = int(m.group(1))
    assert unit == _lib.DUMP_UNIT_SLOTS and unit & (unit - 1) == 0
    assert re.search(r"#define\s+PG_DUMP_MAX_DIGITS\s+18\b", hdr) and _lib.DUMP_MAX_DIGITS == 18
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
    # each entry cites what it stands in for
    assert re.search(r"pg_table_dump_sizes\s+stands in for[^;]*feature\.py:87,103", hdr)
    assert re.search(r"pg_table_dump_text\s+stands in for[^;]*feature\.py:87,103", hdr)
    assert re.search(r"pg_dump_parse\s+stands in for[^;]*count_kmer\.cpp:139-170", hdr)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name) and name in _lib.EXPORTS
    assert _lib.load().pg_abi_version() == _lib.ABI_VERSION == 9


KIND_REFUSALS = [
    (_table(kind=9), "unknown table kind 9"),
    (_table(kind=0), "unknown table kind 0"),
    (_table(kind=_lib.TABLE_DENSE, k=17), "dense table needs 1 <= k <= 16 (got 17)"),
    (_table(kind=_lib.TABLE_HASH, k=22), "hash table needs 1 <= k <= 21 (got 22)"),
    (_table(kind=_lib.TABLE_WIDE, k=32, log2_bucket_slots=0), "wide table needs 1 <= k <= 31 (got 32)"),
    (_table(k=12), "mini table needs 13 <= k <= 21 (got 12)"),
    (_table(kind=_lib.TABLE_MINI_WIDE, k=21), "wide mini table needs 21 < k <= 31 (got 21)"),
]


@pytest.mark.parametrize("args,text", [
    ((None, 1, FAKE, FAKE), "pg_table_dump_sizes: t is null"),
    ((_table(), 1, None, FAKE), "pg_table_dump_sizes: unit_bytes is null"),
    ((_table(), 0, FAKE, FAKE), "pg_table_dump_sizes: lower is below 1 (0)"),
    ((_table(), -4, FAKE, None), "pg_table_dump_sizes: lower is below 1 (-4)"),
    ((_table(data=FAKE + 8), 1, FAKE, None), "pg_table_dump_sizes: t->data is not 16-byte aligned"),
] + [((t, 1, FAKE, None), text) for t, text in KIND_REFUSALS])
def test_dump_sizes_refusals(args, text):
    rc, msg = _call("pg_table_dump_sizes", _ref(args[0]), *args[1:], None)
    assert rc == EINVAL and msg == text


# (t, lower, unit_begin, unit_end, unit_offsets, text_base, range_bytes, text, text_bytes); a table of 2^20 slots has 1024 units
@pytest.mark.parametrize("args,text", [
    ((None, 1, 0, 1, FAKE, 0, 64, FAKE, 64), "pg_table_dump_text: t is null"),
    ((_table(), 1, 0, 1, None, 0, 64, FAKE, 64), "pg_table_dump_text: unit_offsets is null"),
    ((_table(), 1, 0, 1, FAKE, 0, 64, None, 64), "pg_table_dump_text: text is null"),
    ((_table(), 0, 0, 1, FAKE, 0, 64, FAKE, 64), "pg_table_dump_text: lower is below 1 (0)"),
    ((_table(), 1, 0, 1, FAKE, -1, 64, FAKE, 64), "pg_table_dump_text: text_base is negative (-1)"),
    ((_table(), 1, 0, 1, FAKE, 0, -64, FAKE, 64), "pg_table_dump_text: range_bytes is negative (-64)"),
    ((_table(), 1, 0, 1, FAKE, 0, 0, FAKE, -1), "pg_table_dump_text: text_bytes is negative (-1)"),
    ((_table(), 1, 3, 2, FAKE, 0, 64, FAKE, 64), "pg_table_dump_text: units [3, 2) are no range"),
    ((_table(), 1, -1, 2, FAKE, 0, 64, FAKE, 64), "pg_table_dump_text: units [-1, 2) are no range"),
    ((_table(), 1, 0, 1025, FAKE, 0, 64, FAKE, 64), "pg_table_dump_text: units [0, 1025) reach past the table's 1024"),
    ((_table(kind=_lib.TABLE_DENSE, k=3), 1, 0, 2, FAKE, 0, 64, FAKE, 64), "pg_table_dump_text: units [0, 2) reach past the table's 1"),
    # the offsets as the host knows them: units [4, 9) hold 1000 bytes of text, the buffer 999
    ((_table(), 1, 4, 9, FAKE, 5000, 1000, FAKE, 999), "pg_table_dump_text: text of 999 bytes is shorter than the range's 1000"),
    ((_table(data=FAKE + 4), 1, 0, 1, FAKE, 0, 64, FAKE, 64), "pg_table_dump_text: t->data is not 16-byte aligned"),
] + [((t, 1, 0, 1, FAKE, 0, 64, FAKE, 64), text) for t, text in KIND_REFUSALS])
def test_dump_text_refusals(args, text):
    rc, msg = _call("pg_table_dump_text", _ref(args[0]), *args[1:], None)
    assert rc == EINVAL and msg == text


# (text, n_bytes, k, first_ordinal, codes, counts, ordinals, cap, n_out, status, workspace, workspace_bytes)
@pytest.mark.parametrize("args,text", [
    ((None, 64, 21, 0, FAKE, FAKE, FAKE, 8, FAKE, FAKE, FAKE, 4096), "pg_dump_parse: text is null"),
    ((FAKE, -1, 21, 0, FAKE, FAKE, FAKE, 8, FAKE, FAKE, FAKE, 4096), "pg_dump_parse: n_bytes is negative (-1)"),
    ((FAKE, 64, 0, 0, FAKE, FAKE, FAKE, 8, FAKE, FAKE, FAKE, 4096), "pg_dump_parse: k 0 outside [1, 31]"),
    ((FAKE, 64, 32, 0, FAKE, FAKE, FAKE, 8, FAKE, FAKE, FAKE, 4096), "pg_dump_parse: k 32 outside [1, 31]"),
    ((FAKE, 64, 21, -2, FAKE, FAKE, FAKE, 8, FAKE, FAKE, FAKE, 4096), "pg_dump_parse: first_ordinal is negative (-2)"),
    ((FAKE, 64, 21, 0, None, FAKE, FAKE, 8, FAKE, FAKE, FAKE, 4096), "pg_dump_parse: codes is null"),
    ((FAKE, 64, 21, 0, FAKE, None, FAKE, 8, FAKE, FAKE, FAKE, 4096), "pg_dump_parse: counts is null"),
    ((FAKE, 64, 21, 0, FAKE, FAKE, None, 8, FAKE, FAKE, FAKE, 4096), "pg_dump_parse: ordinals is null"),
    ((FAKE, 64, 21, 0, FAKE, FAKE, FAKE, -8, FAKE, FAKE, FAKE, 4096), "pg_dump_parse: cap is negative (-8)"),
    ((FAKE, 64, 21, 0, FAKE, FAKE, FAKE, 8, None, FAKE, FAKE, 4096), "pg_dump_parse: n_out is null"),
    ((FAKE, 64, 21, 0, FAKE, FAKE, FAKE, 8, FAKE, None, FAKE, 4096), "pg_dump_parse: status is null"),
    ((FAKE + 3, 64, 21, 0, FAKE, FAKE, FAKE, 8, FAKE, FAKE, FAKE, 4096), "pg_dump_parse: text is not 16-byte aligned"),
    ((FAKE, 64, 21, 0, FAKE, FAKE, FAKE, 8, FAKE, FAKE, None, 4096), "pg_dump_parse: workspace of 4096 bytes, 32 needed (8-byte aligned)"),
    ((FAKE, 64, 21, 0, FAKE, FAKE, FAKE, 8, FAKE, FAKE, FAKE, 31), "pg_dump_parse: workspace of 31 bytes, 32 needed (8-byte aligned)"),
    ((FAKE, 4097, 21, 0, FAKE, FAKE, FAKE, 8, FAKE, FAKE, FAKE + 4, 4096), "pg_dump_parse: workspace of 4096 bytes, 48 needed (8-byte aligned)"),
])
def test_dump_parse_refusals(args, text):
    rc, msg = _call("pg_dump_parse", *args, None)
    assert rc == EINVAL and msg == text


def test_nothing_to_do_is_ok_and_launches_nothing():
    for t in (_table(), _table(kind=_lib.TABLE_MINI_WIDE, k=25), _table(kind=_lib.TABLE_HASH, log2_bucket_slots=0),
              _table(kind=_lib.TABLE_WIDE, k=31, log2_bucket_slots=0), _table(kind=_lib.TABLE_DENSE, k=4)):
        assert _call("pg_table_dump_text", C.byref(t), 1, 1, 1, FAKE, 0, 0, FAKE, 0, None)[0] == OK       # an empty unit range
        assert _call("pg_table_dump_text", C.byref(t), 1, 0, 1, FAKE, 0, 0, FAKE, 0, None)[0] == OK       # units without text
    assert _call("pg_dump_parse", FAKE, 0, 21, 0, FAKE, FAKE, FAKE, 0, FAKE, FAKE, None, 0, None)[0] == OK
    L = _lib.load()
    assert L.pg_table_dump_units(C.byref(_table())) == (1 << 20) // _lib.DUMP_UNIT_SLOTS
    assert L.pg_table_dump_units(C.byref(_table(kind=_lib.TABLE_DENSE, k=2))) == 1
    assert L.pg_table_dump_units(C.byref(_table(kind=_lib.TABLE_DENSE, k=8))) == 4 ** 8 // _lib.DUMP_UNIT_SLOTS
    assert L.pg_table_dump_units(C.byref(_table(kind=7))) == EINVAL
    assert L.pg_dump_parse_workspace_bytes(0) == 16 and L.pg_dump_parse_workspace_bytes(4096) == 32 and L.pg_dump_parse_workspace_bytes(-1) == EINVAL


def test_python_faces_refuse_before_touching_a_gpu(tmp_path):
    import torch
    with pytest.raises(ValueError, match="k-mer size 32"):
        kmer.KmerTable.from_dump(str(tmp_path / "never_opened.dump"), 32, "cuda:0")
    with pytest.raises(RuntimeError, match="no CPU path"):
        kmer.KmerTable.from_dump(str(tmp_path / "never_opened.dump"), 21, "cpu")
    t = kmer.KmerTable(4, "dense", torch.zeros(256, dtype=torch.int32))
    with pytest.raises(ValueError, match="at least 1"):
        t.write_dump(str(tmp_path / "x.dump"), lower=0)
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        t.write_dump(str(tmp_path / "x.dump"))
    assert not os.listdir(tmp_path)
    # the device form of key42 (what from_items applies to codes that are on the device already) is the host's
    import numpy as np
    codes = np.concatenate([np.random.RandomState(5).randint(0, 1 << 42, 4096, dtype=np.int64), [0, (1 << 42) - 1]]).astype(np.uint64)
    assert np.array_equal(kmer.key42_torch(torch.from_numpy(codes.view(np.int64))).numpy().view(np.uint64), kmer.key42(codes))


def _main(argv):
    try:
        return cli.main_kmer_table(argv)
    except SystemExit as e:
        return e.code


@pytest.mark.parametrize("argv,text", [
    (["dump", "-k", "21", "-o", "unused.dump"], "no input"),
    (["dump", "-1", "only_one.fq", "-k", "21", "-o", "unused.dump"], "no input"),
    (["dump", "-i", "never_opened.fq", "-k", "0", "-o", "unused.dump"], "k-mer size 0 unsupported"),
    (["dump", "-i", "never_opened.fq", "-k", "32", "-o", "unused.dump"], "k-mer size 32 unsupported"),
    (["dump", "-i", "never_opened.fq", "-k", "21", "-L", "0", "-o", "unused.dump"], "-L must be at least 1"),
    (["dump", "-g", "never_opened.dump", "-k", "21", "-L=-3", "-o", "unused.dump"], "-L must be at least 1"),
    (["dump", "-i", "never_opened.fq", "-k", "21"], "-o"),                          # no output named
])
def test_kmer_table_dump_bad_arguments_exit_1(argv, text, capsys, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    assert _main(argv) == 1
    out = capsys.readouterr()
    assert out.out == "" and "kmer_table" in out.err and text in out.err
    assert not os.listdir(tmp_path)
