"""The depth entries (pg_table_profile, pg_table_depth: `jellyfish query -s` on the table of src/feature.py:87, and the k-mer depth
that stands beside scripts/bin_assembly.sh:43) as far as the host decides about them: declared, exported, mirrored in ``_lib``, and
every refusal returned BEFORE the first HIP call -- the descriptors and buffers carry fake addresses that are never dereferenced --
plus the FASTA reader and the argument handling of ``kmer_table depth``.  No kernel is launched."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

from pangaea_amd import _lib, cli
from pangaea_amd.reads import ReadStream

from .conftest import ROOT

OK, EINVAL = 0, -1
FAKE = 0x7F0000000000            # a 256-byte aligned address that belongs to nobody
HEAD = 256                       # pg_table_depth_workspace_bytes(0, 0)


def _table(kind=_lib.TABLE_MINI, k=21, log2_slots=20, log2_bucket_slots=10, data=FAKE):
    return _lib.pg_table(kind, k, log2_slots, log2_bucket_slots, data)


def _call(name, *args):
    L = _lib.load()
    rc = getattr(L, name)(*args)
    return rc, L.pg_last_error().decode()


def _define(hdr, name):
    m = re.search(r"#define\s+" + name + r"\s+(.+?)\s*(/\*|$)", hdr, flags=re.M)
    assert m, name
    return eval(m.group(1).replace("u", ""))            # (integer literals and shifts only)


def test_header_declares_library_exports_and_lib_mirrors():
    hdr = open(os.path.join(ROOT, "include", "pangaea_feat.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+9\b", hdr) and _lib.ABI_VERSION == 9 and _lib.load().pg_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+pg_table_profile\s*\(\s*const pg_table \*t,\s*const uint64_t \*codes,\s*const uint32_t \*valid,\s*int64_t n_chars,\s*"
                     r"int64_t char_begin,\s*int64_t char_end,\s*uint32_t \*counts\s*,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+pg_table_depth\s*\(\s*const pg_table \*t,\s*const uint64_t \*codes,\s*const uint32_t \*valid,\s*int64_t n_chars,\s*"
                     r"const int64_t \*range_start,\s*const int64_t \*range_end,\s*int64_t n_ranges,\s*int64_t lower,\s*int64_t \*out\s*,\s*"
                     r"void \*workspace,\s*int64_t workspace_bytes,\s*uint32_t \*status,\s*void \*stream\s*\)", code)
    assert re.search(r"int64_t\s+pg_table_depth_workspace_bytes\s*\(\s*int64_t n_long,\s*int64_t long_positions\s*\)", code)
    # each entry cites what it stands in for
    assert re.search(r"pg_table_profile\s+stands in for `jellyfish query -s FILE` on feature\.py:87", hdr)
    assert re.search(r"pg_table_depth\s+stands beside[^;]*scripts/bin_assembly\.sh:43[^;]*scripts/low_abd_reads\.sh:10", hdr)
    assert "2^32 - 1 cannot be told from that" in hdr[hdr.index("pg_table_profile  stands in for"):hdr.index("pg_table_depth    stands beside")]
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("pg_table_profile", "pg_table_depth", "pg_table_depth_workspace_bytes"):
        assert hasattr(raw, name) and name in _lib.EXPORTS
    for name, mine in (("PG_PROFILE_NONE", _lib.PROFILE_NONE), ("PG_DEPTH_SHORT_MAX", _lib.DEPTH_SHORT_MAX), ("PG_DEPTH_MAX_LONG", _lib.DEPTH_MAX_LONG),
                       ("PG_STATUS_DEPTH_WORKSPACE", _lib.STATUS_DEPTH_WORKSPACE), ("PG_DEPTH_N_KMERS", _lib.DEPTH_N_KMERS),
                       ("PG_DEPTH_N_PRESENT", _lib.DEPTH_N_PRESENT), ("PG_DEPTH_SUM", _lib.DEPTH_SUM), ("PG_DEPTH_MAX", _lib.DEPTH_MAX),
                       ("PG_DEPTH_MEDIAN", _lib.DEPTH_MEDIAN)):
        assert _define(hdr, name) == mine, name
    assert _lib.PROFILE_NONE == 0xFFFFFFFF and _lib.DEPTH_SHORT_MAX % 64 == 0
    # the new status bit is none of the old ones
    assert _lib.STATUS_DEPTH_WORKSPACE not in (_lib.STATUS_TABLE_FULL, _lib.STATUS_OVERFLOW_LIST, _lib.STATUS_PLAN_MISMATCH, _lib.STATUS_BOUNDS)


def test_workspace_bytes():
    L = _lib.load()
    assert L.pg_table_depth_workspace_bytes(0, 0) == HEAD
    # 4 bytes per position of the long ranges and 32 per long range behind the head, in units of 256
    assert L.pg_table_depth_workspace_bytes(1, 56) == HEAD + 256
    assert L.pg_table_depth_workspace_bytes(1, 57) == HEAD + 512
    assert L.pg_table_depth_workspace_bytes(3, 1_000_000) == HEAD + (4_000_000 + 96 + 255) // 256 * 256
    n = 6 * 10 ** 9
    assert 4 * n < L.pg_table_depth_workspace_bytes(1, n) <= 4 * n + HEAD + 32 + 255
    for bad in ((-1, 0), (0, -1), (_lib.DEPTH_MAX_LONG + 1, 1 << 40)):
        assert L.pg_table_depth_workspace_bytes(*bad) == EINVAL
    assert L.pg_table_depth_workspace_bytes(_lib.DEPTH_MAX_LONG, 1 << 34) > 0


@pytest.mark.parametrize("args,text", [
    ((None, FAKE, FAKE, 100, 0, 100, FAKE), "pg_table_profile: t is null"),
    ((_table(), None, FAKE, 100, 0, 100, FAKE), "pg_table_profile: the stream is null"),
    ((_table(), FAKE, None, 100, 0, 100, FAKE), "pg_table_profile: the stream is null"),
    ((_table(), FAKE, FAKE, 100, 0, 100, None), "pg_table_profile: counts is null"),
    ((_table(), FAKE, FAKE, -1, 0, 0, FAKE), "pg_table_profile: n_chars is negative (-1)"),
    ((_table(), FAKE, FAKE, 100, -1, 100, FAKE), "pg_table_profile: range [-1, 100) outside the stream's 100 characters"),
    ((_table(), FAKE, FAKE, 100, 0, 101, FAKE), "pg_table_profile: range [0, 101) outside the stream's 100 characters"),
    ((_table(), FAKE, FAKE, 100, 51, 50, FAKE), "pg_table_profile: range [51, 50) outside the stream's 100 characters"),
    ((_table(kind=9), FAKE, FAKE, 100, 0, 100, FAKE), "unknown table kind 9"),
    ((_table(kind=_lib.TABLE_DENSE, k=17), FAKE, FAKE, 100, 0, 100, FAKE), "dense table needs 1 <= k <= 16 (got 17)"),
    ((_table(kind=_lib.TABLE_HASH, k=22), FAKE, FAKE, 100, 0, 100, FAKE), "hash table needs 1 <= k <= 21 (got 22)"),
    ((_table(kind=_lib.TABLE_WIDE, k=32, log2_bucket_slots=0), FAKE, FAKE, 100, 0, 100, FAKE), "wide table needs 1 <= k <= 31 (got 32)"),
    ((_table(k=12), FAKE, FAKE, 100, 0, 100, FAKE), "mini table needs 13 <= k <= 21 (got 12)"),
    ((_table(kind=_lib.TABLE_MINI_WIDE, k=21), FAKE, FAKE, 100, 0, 100, FAKE), "wide mini table needs 21 < k <= 31 (got 21)"),
    ((_table(data=None), FAKE, FAKE, 100, 0, 100, FAKE), "table descriptor is null"),
])
def test_profile_refusals(args, text):
    t = args[0]
    rc, msg = _call("pg_table_profile", None if t is None else C.byref(t), *args[1:], None)
    assert rc == EINVAL and msg == text


# (t, codes, valid, n_chars, range_start, range_end, n_ranges, lower, out, workspace, workspace_bytes, status)
_GOOD = (_table(), FAKE, FAKE, 1000, FAKE, FAKE, 4, 1, FAKE, FAKE, 4096, FAKE)


def _with(**kw):
    names = ("t", "codes", "valid", "n_chars", "range_start", "range_end", "n_ranges", "lower", "out", "workspace", "workspace_bytes", "status")
    return tuple(kw.get(n, v) for n, v in zip(names, _GOOD))


@pytest.mark.parametrize("args,text", [
    (_with(t=None), "pg_table_depth: t is null"),
    (_with(codes=None), "pg_table_depth: the stream is null"),
    (_with(valid=None), "pg_table_depth: the stream is null"),
    (_with(n_chars=-5), "pg_table_depth: n_chars is negative (-5)"),
    (_with(n_chars=1 << 37), "pg_table_depth: a stream of 137438953472 characters is too long"),
    (_with(n_ranges=-1), "pg_table_depth: n_ranges is negative (-1)"),
    (_with(range_start=None), "pg_table_depth: the range arrays are null"),
    (_with(range_end=None), "pg_table_depth: the range arrays are null"),
    (_with(out=None), "pg_table_depth: out is null"),
    (_with(lower=0), "pg_table_depth: lower must be at least 1 (got 0)"),
    (_with(lower=-3), "pg_table_depth: lower must be at least 1 (got -3)"),
    (_with(workspace=None), "pg_table_depth: workspace is null"),
    (_with(workspace=FAKE + 128), "pg_table_depth: workspace is not 256-byte aligned"),
    (_with(workspace=FAKE + 8), "pg_table_depth: workspace is not 256-byte aligned"),
    (_with(workspace_bytes=255), "pg_table_depth: workspace of 255 bytes is smaller than the 256 every call needs"),
    (_with(workspace_bytes=0), "pg_table_depth: workspace of 0 bytes is smaller than the 256 every call needs"),
    (_with(workspace_bytes=-1), "pg_table_depth: workspace of -1 bytes is smaller than the 256 every call needs"),
    (_with(status=None), "pg_table_depth: status is null"),
    (_with(t=_table(kind=7)), "unknown table kind 7"),
    (_with(t=_table(kind=_lib.TABLE_DENSE, k=0)), "dense table needs 1 <= k <= 16 (got 0)"),
    (_with(t=_table(kind=_lib.TABLE_WIDE, k=40, log2_bucket_slots=0)), "wide table needs 1 <= k <= 31 (got 40)"),
    (_with(t=_table(k=30)), "mini table needs 13 <= k <= 21 (got 30)"),
    (_with(t=_table(kind=_lib.TABLE_MINI_WIDE, k=13)), "wide mini table needs 21 < k <= 31 (got 13)"),
    (_with(t=_table(data=None)), "table descriptor is null"),
])
def test_depth_refusals(args, text):
    t = args[0]
    rc, msg = _call("pg_table_depth", None if t is None else C.byref(t), *args[1:], None)
    assert rc == EINVAL and msg == text


@pytest.mark.parametrize("t", [_table(), _table(kind=_lib.TABLE_MINI_WIDE, k=25), _table(kind=_lib.TABLE_HASH, log2_bucket_slots=0),
                               _table(kind=_lib.TABLE_WIDE, k=31, log2_bucket_slots=0), _table(kind=_lib.TABLE_DENSE, k=4)])
def test_nothing_asked_is_ok_and_launches_nothing(t):
    assert _call("pg_table_profile", C.byref(t), FAKE, FAKE, 100, 40, 40, FAKE, None)[0] == OK
    assert _call("pg_table_profile", C.byref(t), FAKE, FAKE, 0, 0, 0, FAKE, None)[0] == OK
    assert _call("pg_table_depth", C.byref(t), FAKE, FAKE, 100, None, None, 0, 1, None, FAKE, HEAD, FAKE, None)[0] == OK


# ------------------------------------------------------------------------------------------------------------ FASTA

FASTA = (b">one first record\r\nACGTACGT\r\nacgtnn\r\n"         # CRLF, two lines, lower case and n
         b">two\n"                                             # an empty record
         b">three\tIUPAC and a blank line\nACGTRYKMSWACGT\n\nBDHVNACGT\n"
         b">\nGATTACA\n"                                       # a header without a name
         b">five|x 5\nGGGGCCCC\nTTTTAAAA\nAC")                 # no final newline
WANT = [("one", b"ACGTACGTacgtnn"), ("two", b""), ("three", b"ACGTRYKMSWACGTBDHVNACGT"), ("", b"GATTACA"), ("five|x", b"GGGGCCCCTTTTAAAAAC")]


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "gz"])
def test_from_fasta_on_the_host(tmp_path, packed):
    path = tmp_path / ("seqs.fa.gz" if packed else "seqs.fa")
    path.write_bytes(gzip.compress(FASTA) if packed else FASTA)
    assert ReadStream.parse_fasta(str(path)) == WANT
    s = ReadStream.from_fasta(str(path))
    assert s.run_names == [n for n, _ in WANT]
    assert np.array_equal(s.run_off, np.concatenate([[0], np.cumsum([len(q) + 1 for _, q in WANT])]))
    assert s.n_chars == int(s.run_off[-1]) and s.codes.device.type == "cpu"
    # every record is followed by one character that is no base; lower case only counts under the lenient plane
    text = b"".join(q + b"N" for _, q in WANT)
    strict = bytes(c if c in b"ACGT" else ord("N") for c in text)
    lenient = bytes(c if c in b"ACGT" else ord("N") for c in text.upper().replace(b"n", b"N"))
    assert s.decode() == strict and s.decode(plane=s.lenient_valid()) == lenient and strict != lenient
    same = ReadStream.from_runs([(n, q + b"N") for n, q in WANT])
    assert np.array_equal(same.codes.numpy(), s.codes.numpy()) and np.array_equal(same.valid.numpy(), s.valid.numpy())
    assert np.array_equal(same.valid_lower.numpy(), s.valid_lower.numpy())


def test_from_fasta_of_nothing_and_of_no_fasta(tmp_path):
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    s = ReadStream.from_fasta(str(empty))
    assert s.n_chars == 0 and s.run_names == [] and s.run_off.tolist() == [0]
    headless = tmp_path / "headless.fa"
    headless.write_bytes(b"ACGT\n>late\nACGT\n")
    with pytest.raises(ValueError, match="in front of the first '>'"):
        ReadStream.from_fasta(str(headless))


# ------------------------------------------------------------------------------------------------------------ the tool

def _main(argv):
    try:
        return cli.main_kmer_table(argv)
    except SystemExit as e:
        return e.code


@pytest.mark.parametrize("argv", [
    ["depth", "-i", "never_opened.fq", "-k", "21", "-o", "unused.tsv"],                                          # no -s
    ["depth", "-k", "21", "-s", "never_opened.fa", "-o", "unused.tsv"],                                          # no table source
    ["depth", "-1", "only_one.fq", "-k", "21", "-s", "never_opened.fa", "-o", "unused.tsv"],
    ["depth", "-i", "a.fq", "-g", "a.dump", "-k", "21", "-s", "never_opened.fa", "-o", "unused.tsv"],            # two table sources
    ["depth", "-1", "a.fq", "-2", "b.fq", "-g", "a.dump", "-k", "21", "-s", "never_opened.fa", "-o", "unused.tsv"],
    ["depth", "-i", "a.fq", "-1", "a.fq", "-2", "b.fq", "-k", "21", "-s", "never_opened.fa", "-o", "unused.tsv"],
    ["depth", "-g", "a.dump", "-k", "21", "-s", "never_opened.fa"],                                              # no -o
    ["depth", "-g", "a.dump", "-k", "21", "-s", "never_opened.fa", "-L", "0", "-o", "unused.tsv"],
    ["depth", "-g", "a.dump", "-k", "40", "-s", "never_opened.fa", "-o", "unused.tsv"],
    ["depth", "-g", "a.dump", "-s", "never_opened.fa", "-o", "unused.tsv"],                                      # no -k
    ["depth", "-g", "never_opened.dump", "-k", "21", "-s", "not_there.fa", "-o", "unused.tsv"],                  # the sequences do not exist
])
def test_kmer_table_depth_bad_arguments_exit_1(argv, capsys, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    assert _main(argv) == 1
    out = capsys.readouterr()
    assert out.out == "" and "kmer_table" in out.err
    assert not os.listdir(tmp_path)
