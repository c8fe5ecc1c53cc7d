"""The three table-combine entries (pg_table_combine_aligned, pg_table_combine_items, pg_table_compare: two tables of
src/feature.py:76-94 met by min, max, diff, left, only or keep) as far as the host decides about them: declared, exported, and every
refusal returned BEFORE anything is enqueued -- the descriptors carry fake addresses that are never dereferenced -- plus the
argument handling of `kmer_table combine`, `kmer_table compare` and `kmer_table dump -U`.  No kernel is launched."""
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
NAMES = ("pg_table_combine_aligned", "pg_table_combine_items", "pg_table_compare")
MIN, MAX, DIFF, LEFT, ONLY, KEEP = range(6)


def _table(kind=_lib.TABLE_MINI, k=21, log2_slots=20, log2_bucket_slots=10, data=FAKE):
    return _lib.pg_table(kind, k, log2_slots, log2_bucket_slots, data)


def _hash(k=21, log2_slots=20, log2_bucket_slots=10, data=FAKE):
    return _table(_lib.TABLE_HASH, k, log2_slots, log2_bucket_slots, data)


def _ref(t):
    return None if t is None else C.byref(t)


def test_header_declares_and_library_exports_the_three_entries():
    hdr = open(os.path.join(ROOT, "include", "pangaea_feat.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+9\b", hdr)                       # additive: the version stays
    assert _lib.ABI_VERSION == 9 and _lib.load().pg_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+pg_table_combine_aligned\s*\(\s*const pg_table \*dst,\s*const pg_table \*a,\s*const pg_table \*b\s*,\s*int op,\s*"
                     r"int64_t lower,\s*int64_t upper\s*,\s*uint32_t \*status,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+pg_table_combine_items\s*\(\s*const pg_table \*a,\s*const pg_table \*b\s*,\s*int op,\s*int64_t lower,\s*int64_t upper,\s*"
                     r"uint64_t \*codes,\s*uint32_t \*counts,\s*int64_t cap,\s*int64_t \*n_out\s*,\s*uint32_t \*status,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+pg_table_compare\s*\(\s*const pg_table \*a,\s*const pg_table \*b\s*,\s*uint64_t \*out\s*,\s*void \*stream\s*\)", code)
    for i, name in enumerate(("MIN", "MAX", "DIFF", "LEFT", "ONLY", "KEEP")):
        assert re.search(rf"#define\s+PG_COMBINE_{name}\s+{i}\b", hdr) and getattr(_lib, f"COMBINE_{name}") == i
    assert _lib.COMBINE_OPS == {"min": MIN, "max": MAX, "diff": DIFF, "left": LEFT, "only": ONLY, "keep": KEEP}
    # each entry says which reference lines it stands beside, and that it replaces none of them
    for name in NAMES:
        assert re.search(name + r"\s+stands beside[^;]*feature\.py:76-94[^;]*replaces\s+nothing of the reference", hdr), name
    assert "count_kmer.cpp:139-170" in hdr[hdr.index("Combining finished tables"):]
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int
    assert len(L.pg_table_combine_aligned.argtypes) == 8 and len(L.pg_table_combine_items.argtypes) == 11 and len(L.pg_table_compare.argtypes) == 4


def _aligned(dst, a, b, op=MIN, lower=1, upper=-1, status=FAKE):
    L = _lib.load()
    rc = L.pg_table_combine_aligned(_ref(dst), _ref(a), _ref(b), op, lower, upper, status, None)
    return rc, L.pg_last_error().decode()


def _items(a, b, op=MIN, lower=1, upper=-1, codes=FAKE, counts=OTHER, cap=16, n_out=THIRD, status=FAKE):
    L = _lib.load()
    rc = L.pg_table_combine_items(_ref(a), _ref(b), op, lower, upper, codes, counts, cap, n_out, status, None)
    return rc, L.pg_last_error().decode()


def _compare(a, b, out=FAKE):
    L = _lib.load()
    rc = L.pg_table_compare(_ref(a), _ref(b), out, None)
    return rc, L.pg_last_error().decode()


A, B, D = dict(data=FAKE), dict(data=OTHER), dict(data=THIRD)


@pytest.mark.parametrize("dst,a,b,kw,text", [
    (None, _table(**A), _table(**B), {}, "pg_table_combine_aligned: dst is null"),
    (_table(**D), None, _table(**B), {}, "pg_table_combine_aligned: a is null"),
    (_table(**D), _table(**A), None, {}, "pg_table_combine_aligned: b is null (only PG_COMBINE_KEEP takes none)"),
    (_table(**D), _table(**A), _table(**B), dict(status=None), "pg_table_combine_aligned: status is null"),
    (_table(**D), _table(**A), _table(**B), dict(op=KEEP), "pg_table_combine_aligned: PG_COMBINE_KEEP takes no b"),
    (_table(**D), _table(**A), _table(**B), dict(op=6), "pg_table_combine_aligned: unknown op 6"),
    (_table(**D), _table(**A), _table(**B), dict(op=-1), "pg_table_combine_aligned: unknown op -1"),
    (_table(**D), _table(**A), _table(**B), dict(lower=0), "pg_table_combine_aligned: lower is below 1 (0)"),
    (_table(**D), _table(**A), _table(**B), dict(lower=5, upper=4), "pg_table_combine_aligned: upper 4 is below lower 5"),
    (_table(**D), _table(**A), _table(**B), dict(lower=2, upper=0), "pg_table_combine_aligned: upper 0 is below lower 2"),
    (_table(**D), _table(data=None), _table(**B), {}, "table descriptor is null"),
    (_table(data=None), _table(**A), _table(**B), {}, "table descriptor is null"),
    (_table(**D), _table(**A), _table(k=15, **B), {}, "pg_table_combine_aligned: k differs (a 21, b 15)"),
    (_table(k=15, **D), _table(**A), _table(**B), {}, "pg_table_combine_aligned: k differs (dst 15, a 21)"),
    # a kind that does not admit k
    (_table(**D), _table(k=22, **A), _table(k=22, **B), {}, "mini table needs 13 <= k <= 21 (got 22)"),
    (_hash(**D), _hash(**A), _hash(k=22, **B), {}, "hash table needs 1 <= k <= 21 (got 22)"),
    (_table(**D), _table(kind=9, **A), _table(**B), {}, "unknown table kind 9"),
    # differing geometry, differing kinds, kinds the aligned form does not take
    (_table(**D), _table(**A), _table(log2_slots=21, **B), {}, "of one geometry"),
    (_table(**D), _table(log2_bucket_slots=11, **A), _table(**B), {}, "of one geometry"),
    (_table(log2_slots=21, **D), _table(**A), None, dict(op=KEEP), "of one geometry"),
    (_table(**D), _table(**A), _hash(**B), {}, "of one geometry"),
    (_hash(**D), _table(**A), _table(**B), {}, "of one geometry"),
    (_hash(log2_bucket_slots=0, **D), _hash(log2_bucket_slots=0, **A), _hash(log2_bucket_slots=0, **B), {}, "of one geometry"),
    (_table(_lib.TABLE_WIDE, 25, 20, 0, THIRD), _table(_lib.TABLE_WIDE, 25, 20, 0, FAKE), _table(_lib.TABLE_WIDE, 25, 20, 0, OTHER), {}, "of one geometry"),
    (_table(_lib.TABLE_DENSE, 8, **D), _table(_lib.TABLE_DENSE, 8, **A), None, dict(op=KEEP), "of one geometry"),
    # alignment, and a destination that is, or overlaps, a source (a == b is fine: see the GPU tests)
    (_table(data=THIRD + 8), _table(**A), _table(**B), {}, "pg_table_combine_aligned: dst->data is not 16-byte aligned"),
    (_table(**D), _table(data=FAKE + 8), _table(**B), {}, "pg_table_combine_aligned: a->data is not 16-byte aligned"),
    (_table(**D), _table(**A), _table(data=OTHER + 8), {}, "pg_table_combine_aligned: b->data is not 16-byte aligned"),
    (_table(**A), _table(**A), _table(**B), {}, "pg_table_combine_aligned: dst aliases a"),
    (_table(data=OTHER + (1 << 20)), _table(**A), _table(**B), {}, "pg_table_combine_aligned: dst aliases b"),
    (_table(**A), _table(**A), None, dict(op=KEEP), "pg_table_combine_aligned: dst aliases a"),
])
def test_combine_aligned_refusals(dst, a, b, kw, text):
    rc, msg = _aligned(dst, a, b, **kw)
    assert rc == EINVAL and text in msg and (msg == text or "of one geometry" in text)


@pytest.mark.parametrize("a,b,kw,text", [
    (None, _table(**B), {}, "pg_table_combine_items: a is null"),
    (_table(**A), None, {}, "pg_table_combine_items: b is null (only PG_COMBINE_KEEP takes none)"),
    (_table(**A), None, dict(op=MAX), "pg_table_combine_items: b is null (only PG_COMBINE_KEEP takes none)"),
    (_table(**A), _table(**B), dict(op=KEEP), "pg_table_combine_items: PG_COMBINE_KEEP takes no b"),
    (_table(**A), _table(**B), dict(status=None), "pg_table_combine_items: status is null"),
    (_table(**A), _table(**B), dict(op=17), "pg_table_combine_items: unknown op 17"),
    (_table(**A), _table(**B), dict(lower=0), "pg_table_combine_items: lower is below 1 (0)"),
    (_table(**A), _table(**B), dict(lower=-3), "pg_table_combine_items: lower is below 1 (-3)"),
    (_table(**A), _table(**B), dict(lower=9, upper=8), "pg_table_combine_items: upper 8 is below lower 9"),
    (_table(**A), _hash(k=15, **B), {}, "pg_table_combine_items: k differs (a 21, b 15)"),
    (_hash(k=25, **A), _table(_lib.TABLE_WIDE, 25, 20, 0, OTHER), {}, "hash table needs 1 <= k <= 21 (got 25)"),
    (_table(_lib.TABLE_WIDE, 25, 20, 0, FAKE), _table(k=25, **B), {}, "mini table needs 13 <= k <= 21 (got 25)"),
    (_table(_lib.TABLE_DENSE, k=21, **A), _table(**B), {}, "dense table needs 1 <= k <= 16 (got 21)"),
    (_table(_lib.TABLE_MINI_WIDE, k=21, log2_bucket_slots=13, **A), None, dict(op=KEEP), "wide mini table needs 21 < k <= 31 (got 21)"),
    (_table(data=None), _table(**B), {}, "table descriptor is null"),
    (_table(**A), _table(data=None), {}, "table descriptor is null"),
    (_table(data=FAKE + 8), _table(**B), {}, "pg_table_combine_items: a->data is not 16-byte aligned"),
    (_table(**A), _hash(data=OTHER + 4), {}, "pg_table_combine_items: b->data is not 16-byte aligned"),
    (_table(**A), _table(**B), dict(cap=-1), "pg_table_combine_items: cap is negative (-1)"),
    (_table(**A), _table(**B), dict(n_out=None), "pg_table_combine_items: n_out is null"),
    (_table(**A), _table(**B), dict(codes=None), "pg_table_combine_items: codes or counts is null"),
    (_table(**A), _table(**B), dict(counts=None), "pg_table_combine_items: codes or counts is null"),
])
def test_combine_items_refusals(a, b, kw, text):
    rc, msg = _items(a, b, **kw)
    assert rc == EINVAL and msg == text


@pytest.mark.parametrize("a,b,out,text", [
    (None, _table(**B), FAKE, "pg_table_compare: a is null"),
    (_table(**A), _table(**B), None, "pg_table_compare: out is null"),
    (_table(**A), _hash(k=11, **B), FAKE, "pg_table_compare: k differs (a 21, b 11)"),
    (_table(k=12, **A), None, FAKE, "mini table needs 13 <= k <= 21 (got 12)"),
    (_table(**A), _table(kind=7, **B), FAKE, "unknown table kind 7"),
    (_table(data=FAKE + 8), None, FAKE, "pg_table_compare: a->data is not 16-byte aligned"),
    (_table(**A), _table(data=OTHER + 8), FAKE, "pg_table_compare: b->data is not 16-byte aligned"),
])
def test_compare_refusals(a, b, out, text):
    rc, msg = _compare(a, b, out)
    assert rc == EINVAL and msg == text


def _main(argv):
    try:
        return cli.main_kmer_table(argv)
    except SystemExit as e:
        return e.code


GA, GB, O = ["-ga", "never_opened.dump"], ["-gb", "nor_this.dump"], ["-o", "unused.dump"]


@pytest.mark.parametrize("argv,text", [
    (["combine", "--op", "min", "-k", "21"] + GA + O, "input B"),                                  # a missing input
    (["combine", "--op", "min", "-k", "21"] + GB + O, "input A"),
    (["combine", "--op", "min", "-k", "21", "-ia", "never_opened.fq"] + O, "input B"),
    (["combine", "--op", "min", "-k", "21", "-ia", "never_opened.fq"] + GA + GB + O, "input A"),   # ... and one given twice
    (["combine", "--op", "sum", "-k", "21"] + GA + GB + O, "--op must be one of min, max, diff, left, only"),
    (["combine", "--op", "keep", "-k", "21"] + GA + GB + O, "--op must be one of"),
    (["combine", "-k", "21"] + GA + GB + O, "--op"),                                               # no op at all
    (["combine", "--op", "min", "-k", "21", "-L", "0"] + GA + GB + O, "-L must be at least 1"),
    (["combine", "--op", "min", "-k", "21", "-L", "5", "-U", "4"] + GA + GB + O, "-U (4) is below -L (5)"),
    (["combine", "--op", "min", "-k", "0"] + GA + GB + O, "k-mer size 0 unsupported"),
    (["combine", "--op", "min", "-k", "32"] + GA + GB + O, "k-mer size 32 unsupported"),
    (["combine", "--op", "min"] + GA + GB + O, "-k"),
    (["combine", "--op", "min", "-k", "21"] + GA + GB, "-o"),
    (["compare", "-k", "21"] + GA, "input B"),
    (["compare", "-k", "21", "-ib", "never_opened.fq"], "input A"),
    (["compare", "-k", "40"] + GA + GB, "k-mer size 40 unsupported"),
    (["compare"] + GA + GB, "-k"),
    (["dump", "-k", "21", "-g", "never_opened.dump", "-L", "0", "-U", "9"] + O, "-L must be at least 1"),
    (["dump", "-k", "21", "-g", "never_opened.dump", "-L", "3", "-U", "2"] + O, "-U (2) is below -L (3)"),
    (["dump", "-k", "21", "-g", "never_opened.dump", "-U", "0"] + O, "-U (0) is below -L (1)"),
    (["dump", "-k", "21", "-U", "7"] + O, "no input"),
])
def test_kmer_table_combine_bad_arguments_exit_1(argv, text, capsys, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    assert _main(argv) == 1
    out = capsys.readouterr()
    assert out.out == "" and "kmer_table" in out.err and text in out.err and "Traceback" not in out.err
    assert not os.listdir(tmp_path)
