"""The barcode-sort entries (pg_fastq_barcode_tags, pg_fastq_tag_keys, pg_fastq_tag_compare: read pairs of a FASTQ text by their
BX:Z: tag, beside src/run_pangaea:237-252) as far as the host decides about them: declared, exported, mirrored in ``_lib``,
every refusal returned BEFORE the first HIP call -- the buffers carry fake addresses that are never dereferenced --, the argument
handling of ``sort_barcodes``, and the reference the GPU tests compare with (tests/_sort_ref.py) on an example whose answer is
written out by hand.  No kernel is launched."""
import ctypes as C
import os
import re

import pytest

from pangaea_amd import _lib, cli

from . import _sort_ref as ref
from .conftest import ROOT

OK, EINVAL = 0, -1
FAKE = 0x7F0000000000            # a 256-byte aligned address that belongs to nobody


def _call(name, *args):
    L = _lib.load()
    rc = getattr(L, name)(*args)
    return rc, L.pg_last_error().decode()


def _define(hdr, name):
    m = re.search(r"#define\s+" + name + r"\s+(.+?)\s*(/\*|$)", hdr, flags=re.M)
    assert m, name
    return eval(m.group(1).replace("ull", "").replace("u", ""))


def test_header_declares_library_exports_and_lib_mirrors():
    hdr = open(os.path.join(ROOT, "include", "pangaea_feat.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+9\b", hdr) and _lib.ABI_VERSION == 9 and _lib.load().pg_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+pg_fastq_barcode_tags\s*\(\s*const uint8_t \*text,\s*int64_t n_bytes,\s*const int64_t \*line_start,\s*int64_t n_units,\s*"
                     r"int lines_per_unit\s*,\s*int64_t \*tag_off\s*,\s*int32_t \*tag_len\s*,\s*uint64_t \*status\s*,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+pg_fastq_tag_keys\s*\(\s*const uint8_t \*text,\s*int64_t n_bytes,\s*const int64_t \*tag_off,\s*const int32_t \*tag_len,\s*"
                     r"const int64_t \*order\s*,\s*int64_t n,\s*int64_t byte_begin,\s*uint64_t \*keys\s*,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+pg_fastq_tag_compare\s*\(\s*const uint8_t \*text,\s*int64_t n_bytes,\s*const int64_t \*tag_off,\s*const int32_t \*tag_len,\s*"
                     r"const int64_t \*order\s*,\s*int64_t n,\s*int8_t \*out\s*,\s*void \*stream\s*\)", code)
    # each entry cites the step of the reference it stands beside
    for name in ("pg_fastq_barcode_tags", "pg_fastq_tag_keys", "pg_fastq_tag_compare"):
        assert re.search(name + r"\s+beside src/run_pangaea:237-252", hdr), name
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("pg_fastq_barcode_tags", "pg_fastq_tag_keys", "pg_fastq_tag_compare"):
        assert hasattr(raw, name) and name in _lib.EXPORTS
        assert getattr(_lib.load(), name).argtypes is not None
    assert _define(hdr, "PG_FASTQ_LONG_TAG") == _lib.FASTQ_LONG_TAG and _define(hdr, "PG_FASTQ_MAX_TAG") == _lib.FASTQ_MAX_TAG == 255
    # the new reason is none of the old ones, and the old ones are what they were
    old = (_lib.FASTQ_NO_AT, _lib.FASTQ_NO_PLUS, _lib.FASTQ_SHORT_QUALITY, _lib.FASTQ_BAD_INDEX)
    assert old == (1, 2, 3, 4) and _lib.FASTQ_LONG_TAG not in old and 0 < _lib.FASTQ_LONG_TAG < 256
    assert [_define(hdr, n) for n in ("PG_FASTQ_NO_AT", "PG_FASTQ_NO_PLUS", "PG_FASTQ_SHORT_QUALITY", "PG_FASTQ_BAD_INDEX")] == [1, 2, 3, 4]


# (text, n_bytes, line_start, n_units, lines_per_unit, tag_off, tag_len, status)
_TAGS = (FAKE, 1000, FAKE, 4, 8, FAKE, FAKE, FAKE)
_TAGS_NAMES = ("text", "n_bytes", "line_start", "n_units", "lines_per_unit", "tag_off", "tag_len", "status")
# (text, n_bytes, tag_off, tag_len, order, n, byte_begin, keys)
_KEYS = (FAKE, 1000, FAKE, FAKE, FAKE, 4, 0, FAKE)
_KEYS_NAMES = ("text", "n_bytes", "tag_off", "tag_len", "order", "n", "byte_begin", "keys")
# (text, n_bytes, tag_off, tag_len, order, n, out)
_CMP = (FAKE, 1000, FAKE, FAKE, FAKE, 4, FAKE)
_CMP_NAMES = ("text", "n_bytes", "tag_off", "tag_len", "order", "n", "out")


def _with(good, names, **kw):
    assert set(kw) <= set(names)
    return tuple(kw.get(n, v) for n, v in zip(names, good))


def _tags(**kw):
    return _with(_TAGS, _TAGS_NAMES, **kw)


def _keys(**kw):
    return _with(_KEYS, _KEYS_NAMES, **kw)


def _cmp(**kw):
    return _with(_CMP, _CMP_NAMES, **kw)


@pytest.mark.parametrize("args,text", [
    (_tags(text=None), "pg_fastq_barcode_tags: text is null"),
    (_tags(line_start=None), "pg_fastq_barcode_tags: line_start is null"),
    (_tags(tag_off=None), "pg_fastq_barcode_tags: tag_off is null"),
    (_tags(tag_len=None), "pg_fastq_barcode_tags: tag_len is null"),
    (_tags(status=None), "pg_fastq_barcode_tags: status is null"),
    (_tags(n_bytes=-1), "pg_fastq_barcode_tags: n_bytes is negative (-1)"),
    (_tags(n_units=-3), "pg_fastq_barcode_tags: n_units is negative (-3)"),
    (_tags(n_units=(1 << 40) + 1), "pg_fastq_barcode_tags: n_units 1099511627777 beyond 2^40"),
    (_tags(lines_per_unit=0), "pg_fastq_barcode_tags: lines_per_unit 0 is neither 4 nor 8"),
    (_tags(lines_per_unit=6), "pg_fastq_barcode_tags: lines_per_unit 6 is neither 4 nor 8"),
    (_tags(lines_per_unit=16), "pg_fastq_barcode_tags: lines_per_unit 16 is neither 4 nor 8"),
    (_tags(text=FAKE + 8), "pg_fastq_barcode_tags: text is not 16-byte aligned"),
])
def test_barcode_tags_refusals(args, text):
    rc, msg = _call("pg_fastq_barcode_tags", *args, None)
    assert rc == EINVAL and msg == text


@pytest.mark.parametrize("args,text", [
    (_keys(text=None), "pg_fastq_tag_keys: text is null"),
    (_keys(tag_off=None), "pg_fastq_tag_keys: tag_off is null"),
    (_keys(tag_len=None), "pg_fastq_tag_keys: tag_len is null"),
    (_keys(keys=None), "pg_fastq_tag_keys: keys is null"),
    (_keys(n_bytes=-1), "pg_fastq_tag_keys: n_bytes is negative (-1)"),
    (_keys(n=-1), "pg_fastq_tag_keys: n is negative (-1)"),
    (_keys(byte_begin=-8), "pg_fastq_tag_keys: byte_begin -8 is no multiple of 8 in [0, 255]"),
    (_keys(byte_begin=4), "pg_fastq_tag_keys: byte_begin 4 is no multiple of 8 in [0, 255]"),
    (_keys(byte_begin=9), "pg_fastq_tag_keys: byte_begin 9 is no multiple of 8 in [0, 255]"),
    (_keys(byte_begin=256), "pg_fastq_tag_keys: byte_begin 256 is no multiple of 8 in [0, 255]"),
    (_keys(text=FAKE + 4), "pg_fastq_tag_keys: text is not 16-byte aligned"),
])
def test_tag_keys_refusals(args, text):
    rc, msg = _call("pg_fastq_tag_keys", *args, None)
    assert rc == EINVAL and msg == text


@pytest.mark.parametrize("args,text", [
    (_cmp(text=None), "pg_fastq_tag_compare: text is null"),
    (_cmp(tag_off=None), "pg_fastq_tag_compare: tag_off is null"),
    (_cmp(tag_len=None), "pg_fastq_tag_compare: tag_len is null"),
    (_cmp(out=None), "pg_fastq_tag_compare: out is null"),
    (_cmp(n_bytes=-7), "pg_fastq_tag_compare: n_bytes is negative (-7)"),
    (_cmp(n=-2), "pg_fastq_tag_compare: n is negative (-2)"),
    (_cmp(text=FAKE + 1), "pg_fastq_tag_compare: text is not 16-byte aligned"),
])
def test_tag_compare_refusals(args, text):
    rc, msg = _call("pg_fastq_tag_compare", *args, None)
    assert rc == EINVAL and msg == text


def test_nothing_to_do_is_ok_and_launches_nothing():
    # (no units: PG_OK before any HIP call, and a null order is the identity, not an error)
    assert _call("pg_fastq_barcode_tags", *_tags(n_units=0), None)[0] == OK
    assert _call("pg_fastq_tag_keys", *_keys(n=0, order=None), None)[0] == OK
    assert _call("pg_fastq_tag_compare", *_cmp(n=0, order=None), None)[0] == OK


def _cli(argv, capsys):
    rc = cli.main_sort_barcodes(argv)
    return rc, capsys.readouterr().err


def test_cli_refuses_bad_arguments(tmp_path, capsys):
    f = str(tmp_path / "a.fq")
    open(f, "w").close()
    out = str(tmp_path / "o.fq")
    assert _cli(["-i", f, "-1", f, "-2", f, "-o", out], capsys) == (1, "sort_barcodes: the reads to sort are -i F or -1 F -2 F (one of the two)\n")
    assert _cli(["-o", out], capsys) == (1, "sort_barcodes: the reads to sort are -i F or -1 F -2 F (one of the two)\n")
    assert _cli(["-i", f], capsys) == (1, "sort_barcodes: -o OUT is needed (or --check)\n")
    assert _cli(["-2", f, "-o", out], capsys) == (1, "sort_barcodes: -1 and -2 go together\n")
    assert _cli(["-1", f, "-o", out], capsys) == (1, "sort_barcodes: -1 and -2 go together\n")
    assert _cli(["--check", "-i", f, "-o", out], capsys) == (2, "sort_barcodes: --check writes nothing: -o does not go with it\n")
    assert _cli(["-i", f, "-o", out + ".gz"], capsys) == (1, f"sort_barcodes: {out}.gz: the sorted reads are written as plain text, gzip output is not supported\n")
    missing = str(tmp_path / "none.fq")
    assert _cli(["-i", missing, "-o", out], capsys) == (1, f"sort_barcodes: {missing}: no such file\n")
    assert _cli(["--check", "-1", f, "-2", missing], capsys) == (2, f"sort_barcodes: {missing}: no such file\n")
    assert not os.path.exists(out)
    with pytest.raises(SystemExit) as e:                     # (an unknown flag: argparse's usage, exit status 1 as the other tools)
        cli.main_sort_barcodes(["--nope"])
    assert e.value.code == 1
    capsys.readouterr()


def _rec(header: bytes, seq: bytes = b"ACGT") -> bytes:
    return header + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"


def test_reference_on_a_hand_written_example():
    # seven pairs; the tag of a pair is that of its FIRST header
    pairs = [
        (b"@p0 BX:Z:ACGT-1", b"@p0 BX:Z:ACGT-1"),
        (b"@p1", b"@p1 BX:Z:AAAA-1"),                        # a tag on R2's header only: untagged
        (b"@p2 BX:Z:AC", b"@p2"),                            # a prefix of p0's tag: in front of it
        (b"@p3 BX:Z: BX:Z:ACGT-1\tx", b"@p3"),               # "BX:Z: " is no match, the later one is; ended by the tab: p0's tag
        (b"@p4 BX:Z:\xff\xff", b"@p4"),                      # bytes >= 0x80 behind every ASCII tag, in front of the untagged
        (b"@p5 BX:Z:~~~~", b"@p5"),                          # beyond the reference's "~~~" and still in front of the untagged
        (b"@p6 BX:Z:AC BX:Z:AAAA", b"@p6"),                  # two tags: the first
    ]
    data = b"".join(_rec(a) + _rec(b, b"TTGA") for a, b in pairs)
    units = ref.units_of(data)
    assert [u[0] for u in units] == [b"BX:Z:ACGT-1", None, b"BX:Z:AC", b"BX:Z:ACGT-1", b"BX:Z:\xff\xff", b"BX:Z:~~~~", b"BX:Z:AC"]
    assert ref.tag_of(b"@p3 BX:Z: BX:Z:ACGT-1\tx") == (10, b"BX:Z:ACGT-1")
    assert ref.tag_of(b"@x BX:Z:") == (-1, None) and ref.tag_of(b"@x BX:Z") == (-1, None) and ref.tag_of(b"@x BX:Z:A\r") == (3, b"BX:Z:A")
    # AC (p2, then p6: input order), ACGT-1 (p0, p3), ~~~~ (p5), 0xFF 0xFF (p4), untagged (p1)
    assert ref.order(units) == [2, 6, 0, 3, 5, 4, 1]
    assert ref.sort_text(data) == b"".join(_rec(pairs[i][0]) + _rec(pairs[i][1], b"TTGA") for i in (2, 6, 0, 3, 5, 4, 1))
    assert ref.barcodes(units) == 4 and ref.runs(units) == 5 and ref.first_descent(units) == 2
    assert ref.first_descent([units[i] for i in ref.order(units)]) is None
    # R1 / R2 files give the same units; a last line without newline gets one, CRLF line ends stay
    r1 = b"".join(_rec(a) for a, _ in pairs)
    r2 = b"".join(_rec(b, b"TTGA") for _, b in pairs)
    assert ref.sort_text(r1, r2) == ref.sort_text(data)
    assert ref.sort_text(data[:-1]) == ref.sort_text(data)
    crlf = data.replace(b"\n", b"\r\n")
    assert ref.sort_text(crlf) == ref.sort_text(data).replace(b"\n", b"\r\n")
    assert ref.sort_text(b"") == b"" and ref.order([]) == [] and ref.runs([]) == 0
