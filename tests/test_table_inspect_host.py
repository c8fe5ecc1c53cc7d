"""The two read-only table entries (pg_table_query, pg_table_spectrum: what `jellyfish query` / `jellyfish histo` give from the
dump of src/feature.py:87,103) as far as the host decides about them: declared, exported, and every refusal returned BEFORE the
first HIP call -- the descriptors carry fake addresses that are never dereferenced -- plus the k-mer encoder and the argument
handling of the `kmer_table` tool.  No kernel is launched."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pangaea_amd import _lib, cli, kmer

from .conftest import ROOT

OK, EINVAL = 0, -1
FAKE = 0x7F0000000000            # a 256-byte aligned address that belongs to nobody


def _table(kind=_lib.TABLE_MINI, k=21, log2_slots=20, log2_bucket_slots=10, data=FAKE):
    return _lib.pg_table(kind, k, log2_slots, log2_bucket_slots, data)


def _call(name, *args):
    L = _lib.load()
    rc = getattr(L, name)(*args)
    return rc, L.pg_last_error().decode()


def test_header_declares_and_library_exports_both_entries():
    hdr = open(os.path.join(ROOT, "include", "pangaea_feat.h")).read()
    assert re.search(r"#define\s+PG_QUERY_INVALID\s+0xFFFFFFFFu", hdr) and re.search(r"#define\s+PG_SPECTRUM_MAX_HIGH\s+16382\b", hdr)
    assert re.search(r"#define\s+PG_ABI_VERSION\s+9\b", hdr)                       # additive: the version stays
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+pg_table_query\s*\(\s*const pg_table \*t,\s*const uint64_t \*codes,\s*int64_t n,\s*uint32_t \*counts,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+pg_table_spectrum\s*\(\s*const pg_table \*t,\s*int high,\s*uint64_t \*hist\s*,\s*void \*stream\s*\)", code)
    # each entry cites what it stands in for
    for name in ("pg_table_query", "pg_table_spectrum"):
        assert re.search(name + r"\s+stands in for[^;]*feature\.py:87", hdr), name
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("pg_table_query", "pg_table_spectrum"):
        assert hasattr(raw, name) and name in _lib.EXPORTS
    assert _lib.QUERY_INVALID == 0xFFFFFFFF and _lib.SPECTRUM_MAX_HIGH == 16382


@pytest.mark.parametrize("args,text", [
    ((None, FAKE, 8, FAKE), "pg_table_query: t is null"),
    ((_table(), None, 8, FAKE), "pg_table_query: codes is null"),
    ((_table(), FAKE, 8, None), "pg_table_query: counts is null"),
    ((_table(), FAKE, -1, FAKE), "pg_table_query: n is negative (-1)"),
    ((_table(kind=9), FAKE, 8, FAKE), "unknown table kind 9"),
    ((_table(kind=0), FAKE, 8, FAKE), "unknown table kind 0"),
    ((_table(kind=_lib.TABLE_DENSE, k=17), FAKE, 8, FAKE), "dense table needs 1 <= k <= 16 (got 17)"),
    ((_table(kind=_lib.TABLE_DENSE, k=0), FAKE, 8, FAKE), "dense table needs 1 <= k <= 16 (got 0)"),
    ((_table(kind=_lib.TABLE_HASH, k=22), FAKE, 8, FAKE), "hash table needs 1 <= k <= 21 (got 22)"),
    ((_table(kind=_lib.TABLE_WIDE, k=32, log2_bucket_slots=0), FAKE, 8, FAKE), "wide table needs 1 <= k <= 31 (got 32)"),
    ((_table(k=12), FAKE, 8, FAKE), "mini table needs 13 <= k <= 21 (got 12)"),
    ((_table(k=22), FAKE, 8, FAKE), "mini table needs 13 <= k <= 21 (got 22)"),
    ((_table(kind=_lib.TABLE_MINI_WIDE, k=21), FAKE, 8, FAKE), "wide mini table needs 21 < k <= 31 (got 21)"),
    ((_table(kind=_lib.TABLE_MINI_WIDE, k=32), FAKE, 8, FAKE), "wide mini table needs 21 < k <= 31 (got 32)"),
])
def test_query_refusals(args, text):
    t = args[0]
    rc, msg = _call("pg_table_query", None if t is None else C.byref(t), *args[1:], None)
    assert rc == EINVAL and msg == text


@pytest.mark.parametrize("args,text", [
    ((None, 100, FAKE), "pg_table_spectrum: t is null"),
    ((_table(), 100, None), "pg_table_spectrum: hist is null"),
    ((_table(), 0, FAKE), "pg_table_spectrum: high 0 outside [1, 16382]"),
    ((_table(), -5, FAKE), "pg_table_spectrum: high -5 outside [1, 16382]"),
    ((_table(), 16383, FAKE), "pg_table_spectrum: high 16383 outside [1, 16382]"),
    ((_table(kind=7), 100, FAKE), "unknown table kind 7"),
    ((_table(kind=_lib.TABLE_DENSE, k=17), 100, FAKE), "dense table needs 1 <= k <= 16 (got 17)"),
    ((_table(kind=_lib.TABLE_HASH, k=0), 100, FAKE), "hash table needs 1 <= k <= 21 (got 0)"),
    ((_table(kind=_lib.TABLE_WIDE, k=40, log2_bucket_slots=0), 100, FAKE), "wide table needs 1 <= k <= 31 (got 40)"),
    ((_table(k=30), 100, FAKE), "mini table needs 13 <= k <= 21 (got 30)"),
    ((_table(kind=_lib.TABLE_MINI_WIDE, k=13), 100, FAKE), "wide mini table needs 21 < k <= 31 (got 13)"),
    ((_table(data=FAKE + 8), 100, FAKE), "pg_table_spectrum: t->data is not 16-byte aligned"),
])
def test_spectrum_refusals(args, text):
    t = args[0]
    rc, msg = _call("pg_table_spectrum", None if t is None else C.byref(t), *args[1:], None)
    assert rc == EINVAL and msg == text


@pytest.mark.parametrize("t", [_table(), _table(kind=_lib.TABLE_MINI_WIDE, k=25), _table(kind=_lib.TABLE_HASH, log2_bucket_slots=0),
                               _table(kind=_lib.TABLE_WIDE, k=31, log2_bucket_slots=0), _table(kind=_lib.TABLE_DENSE, k=4)])
def test_query_of_nothing_is_ok_and_launches_nothing(t):
    rc, _ = _call("pg_table_query", C.byref(t), FAKE, 0, FAKE, None)
    assert rc == OK


def test_encode_kmers():
    assert kmer.encode_kmers(["A", "C", "T", "G"], 1).tolist() == [0, 1, 2, 3]
    got = kmer.encode_kmers(["ACGT", "TTTT", "AAAA", "GATC"], 4)
    assert got.dtype == np.uint64
    # the first character highest, the newest (last) in the low two bits
    assert got.tolist() == [(0 << 6) | (1 << 4) | (3 << 2) | 2, 0b10101010, 0, (3 << 6) | (0 << 4) | (2 << 2) | 1]
    assert int(kmer.encode_kmers(["G" * 31], 31)[0]) == (1 << 62) - 1
    assert kmer.encode_kmers([], 21).shape == (0,) and kmer.encode_kmers([], 21).dtype == np.uint64
    # the same codes as the dump loader's forward strand (cli.load_dump: (c >> 1) & 3, first character highest)
    s = "GATTACAGATTACAGATTACA"
    want = 0
    for ch in s:
        want = (want << 2) | "ACTG".index(ch)
    assert int(kmer.encode_kmers([s], 21)[0]) == want
    for bad in (["ACG"], ["ACGTA"], [""], ["ACGT", "ACG"]):
        with pytest.raises(ValueError, match="length 4"):
            kmer.encode_kmers(bad, 4)
    for bad in (["ACGN"], ["acgt"], ["ACgT"], ["AC-T"], ["ACGé"], ["ACGT", "RCGT"]):
        with pytest.raises(ValueError, match="other than A, C, G, T"):
            kmer.encode_kmers(bad, 4)


def _main(argv):
    try:
        return cli.main_kmer_table(argv)
    except SystemExit as e:
        return e.code


@pytest.mark.parametrize("argv", [
    ["histo", "-k", "21", "-o", "unused.histo"],                                   # no input
    ["query", "-k", "21", "A" * 21],
    ["query", "-1", "only_one.fq", "-k", "21", "A" * 21],
    ["dump", "-i", "x.fq", "-k", "21"],                                            # unknown sub-command
    [],
    ["query", "-i", "never_opened.fq", "-k", "21", "ACGT"],                        # a k-mer of the wrong length
    ["query", "-i", "never_opened.fq", "-k", "4", "ACGT", "ACGN"],                 # ... and one with another character
    ["histo", "-i", "never_opened.fq", "-k", "21", "--high", "0", "-o", "unused.histo"],
    ["histo", "-i", "never_opened.fq", "-k", "40", "-o", "unused.histo"],
])
def test_kmer_table_bad_arguments_exit_1(argv, capsys, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    assert _main(argv) == 1
    out = capsys.readouterr()
    assert out.out == "" and "kmer_table" in out.err
    assert not os.listdir(tmp_path)


def test_kmer_table_launcher_exits_1_without_input():
    tool = os.path.join(ROOT, "pangaea_amd", "bin", "kmer_table")
    assert os.access(tool, os.X_OK)
    r = subprocess.run([sys.executable, tool, "query", "-k", "21", "A" * 20, "-g", "never_opened.dump"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == "" and "length 21" in r.stderr
