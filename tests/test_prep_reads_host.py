"""Raw stLFR / TELL-seq reads brought to the BX:Z: form (pg_fastq_prep_plan, pg_fastq_prep_write; pangaea_amd/prepreads.py) as far
as the host decides about them: the plain-Python restatement of the rules (tests/_prep_ref.py) against the files the reference's
own binaries wrote (tests/golden/prep/, made by tests/golden/make_prep_goldens.py), the entries declared, exported and mirrored
in ``_lib``, every refusal returned BEFORE the first HIP call -- the buffers carry fake addresses that are never dereferenced
--, and the argument handling of ``preprocess_reads`` and ``sort_barcodes --short_type``.  No kernel is launched."""
import ctypes as C
import gzip
import os
import re

import pytest

from pangaea_amd import _lib, cli

from . import _prep_ref as ref
from .conftest import GOLDEN, ROOT

OK, EINVAL = 0, -1
FAKE = 0x7F0000000000            # a 256-byte aligned address that belongs to nobody
PREP = os.path.join(GOLDEN, "prep")


def _golden(name: str) -> bytes:
    with open(os.path.join(PREP, name), "rb") as f:
        return f.read()


def test_restatement_equals_the_reference_binaries_output():
    s = ref.preprocess("stlfr", _golden("stlfr_R1.fq"), _golden("stlfr_R2.fq"))
    assert s["out1"] == _golden("stlfr.ref_1.fq") and s["out2"] == _golden("stlfr.ref_2.fq")
    assert (s["pairs"], s["written"], s["wl"]) == (15, 15, None) and 0 < s["tagged"] < s["pairs"]
    t = ref.preprocess("tellseq", _golden("tellseq_R1.fq"), _golden("tellseq_R2.fq"), _golden("tellseq_I1.fq"))
    assert t["out1"] == _golden("tellseq.ref_1.fq") and t["out2"] == _golden("tellseq.ref_2.fq") and t["wl"] == _golden("tellseq.ref.wl")
    assert (t["pairs"], t["written"], t["tagged"]) == (10, 6, 6)
    # the gzip copies hold the same bytes
    for name in ("stlfr_R1.fq", "stlfr_R2.fq"):
        assert gzip.decompress(_golden(name + ".gz")) == _golden(name)


def test_goldens_cover_what_they_should():
    r1 = ref.records_of(_golden("stlfr_R1.fq"))
    barcodes = [h.split(b"#", 1)[1].split(b"/")[0] for h, *_ in r1]
    # every combination of zero / non-zero fields, and which of them the reference tags (f1 twice, f3 never)
    tagged = {b: ref.stlfr_plan(b"@x#" + b)[2] for b in barcodes}
    assert [tagged[b] for b in (b"5_6_7", b"5_6_0", b"5_0_7", b"5_0_0", b"0_6_7", b"0_6_0", b"0_0_7", b"0_0_0")] == [True, True] + [False] * 6
    assert any(b"/" not in h.split(b"#", 1)[1] for h, *_ in r1)                      # a barcode without '/'
    assert any(b"/1 " in h for h, *_ in r1)                                          # text behind the '/'
    assert any(len(x[2]) > 1 for x in r1) and any(x[1].endswith(b"\r") and x[3].endswith(b"\r") for x in r1)    # +name, CRLF
    lens = [len(x[1]) for x in ref.records_of(_golden("tellseq_I1.fq"))]
    assert {0, 17, 18, 19} <= set(lens)
    index = [x[1] for x in ref.records_of(_golden("tellseq_I1.fq"))]
    assert any(b"N" in b and len(b) == 18 for b in index) and any(b.endswith(b"\r") and len(b) == 19 for b in index)
    heads = [x[0] for x in ref.records_of(_golden("tellseq_R1.fq"))]
    assert any(b" " not in h for h in heads) and any(b"\t" in h.split(b" ")[0] for h in heads) and any(h.find(b" ") == 63 for h in heads)


def _rec(header: bytes, seq: bytes = b"ACGT", third: bytes = b"+") -> bytes:
    return header + b"\n" + seq + b"\n" + third + b"\n" + b"I" * len(seq) + b"\n"


def test_restatement_on_hand_written_examples():
    r1 = _rec(b"@a#1_2_3/1", b"ACGT", b"+a") + _rec(b"@b#0_2_3/1 rest") + _rec(b"@c#7_8_0")
    r2 = _rec(b"@other/2", b"TT") + _rec(b"@b#0_2_3/2", b"GG") + _rec(b"@c#7_8_0", b"CC")
    s = ref.preprocess("stlfr", r1, r2[:-1])                 # (a last line without newline gets one)
    assert s["out1"] == _rec(b"@a\tBX:Z:1_2_3-1", b"ACGT", b"+a") + _rec(b"@b") + _rec(b"@c\tBX:Z:7_8_0-1")
    assert s["out2"] == _rec(b"@a\tBX:Z:1_2_3-1", b"TT") + _rec(b"@b", b"GG") + _rec(b"@c\tBX:Z:7_8_0-1", b"CC")
    assert ref.interleaved(s) == b"".join(a + b for a, b in zip(s["units1"], s["units2"])) and ref.interleaved(s).startswith(s["units1"][0] + s["units2"][0])
    i1 = _rec(b"@a 1", b"A" * 18) + _rec(b"@b 1", b"C" * 17) + _rec(b"@c 1", b"G" * 18 + b"\r")
    t = ref.preprocess("tellseq", _rec(b"@a x y", b"ACGT", b"+a x y") * 3, _rec(b"@a\tz", b"TT") * 3, i1)
    assert t["out1"] == _rec(b"@a\tBX:Z:" + b"A" * 18 + b"-1") and t["out2"] == _rec(b"@a\tBX:Z:" + b"A" * 18 + b"-1", b"TT")
    assert t["wl"] == b"A" * 18 + b"\n" and (t["pairs"], t["tagged"]) == (3, 1)
    for header, reason in ((b"@nohash", ref.NO_HASH), (b"@x#1_2", ref.FEW_FIELDS), (b"@x#12/1_2_3", ref.FEW_FIELDS), (b"@x#" + b"1_2_" + b"3" * 250, ref.LONG_TAG)):
        with pytest.raises(ref.Malformed) as e:
            ref.plan("stlfr", _rec(b"@ok#1_2_3") + _rec(header), _rec(b"@m") * 2)
        assert (e.value.file, e.value.record, e.value.reason) == (0, 1, reason)
    assert ref.plan("stlfr", _rec(b"@x#" + b"1_2_" + b"3" * 249), _rec(b"@m"))[0][2] is True           # 253 bytes pass
    with pytest.raises(ref.Malformed) as e:
        ref.plan("tellseq", _rec(b"@a"), _rec(b"@a"), _rec(b"@a", b"A" * 18, b"-"))
    assert (e.value.file, e.value.record, e.value.reason) == (2, 0, ref.NO_PLUS)


def _define(hdr, name):
    m = re.search(r"#define\s+" + name + r"\s+(.+?)\s*(/\*|$)", hdr, flags=re.M)
    assert m, name
    return eval(m.group(1).replace("ull", "").replace("u", ""))


def test_header_declares_library_exports_and_lib_mirrors():
    hdr = open(os.path.join(ROOT, "include", "pangaea_feat.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+9\b", hdr) and _lib.ABI_VERSION == 9 and _lib.load().pg_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("pg_fastq_prep_plan", "pg_fastq_prep_write"):
        assert re.search(r"int\s+" + name + r"\s*\(\s*int mode\s*,", code), name
        assert hasattr(raw, name) and name in _lib.EXPORTS and getattr(_lib.load(), name).argtypes is not None
    assert re.search(r"pg_fastq_prep_plan\s+beside preprocess_stlfr\.cpp:\d+-\d+ / preprocess_tellseq\.cpp:\d+-\d+", hdr)
    assert re.search(r"pg_fastq_prep_write\s+beside preprocess_stlfr\.cpp:\d+-\d+ / preprocess_tellseq\.cpp:\d+-\d+", hdr)
    assert "preprocess_stlfr.cpp:89" in hdr                   # the oddity that is kept is said where the rule is stated
    assert _define(hdr, "PG_FASTQ_NO_HASH") == _lib.FASTQ_NO_HASH and _define(hdr, "PG_FASTQ_FEW_FIELDS") == _lib.FASTQ_FEW_FIELDS
    assert _define(hdr, "PG_PREP_STLFR") == _lib.PREP_STLFR and _define(hdr, "PG_PREP_TELLSEQ") == _lib.PREP_TELLSEQ
    assert _lib.PREP_MODES == {"stlfr": _lib.PREP_STLFR, "tellseq": _lib.PREP_TELLSEQ}
    # the new reasons are none of the old ones, and the old ones are what they were
    old = (_lib.FASTQ_NO_AT, _lib.FASTQ_NO_PLUS, _lib.FASTQ_SHORT_QUALITY, _lib.FASTQ_BAD_INDEX, _lib.FASTQ_LONG_TAG)
    assert old == (1, 2, 3, 4, 5) and len({*old, _lib.FASTQ_NO_HASH, _lib.FASTQ_FEW_FIELDS}) == 7 and (ref.NO_HASH, ref.FEW_FIELDS) == (6, 7)
    assert _lib.FASTQ_MAX_TAG - 2 == ref.MAX_B


# (mode, text1, n1_bytes, line_start1, text2, n2_bytes, line_start2, text_i, n_i_bytes, line_start_i, n_units, first_unit, head_len,
#  bc_off, bc_len, tagged, status)
_PLAN_NAMES = ("mode", "text1", "n1_bytes", "line_start1", "text2", "n2_bytes", "line_start2", "text_i", "n_i_bytes", "line_start_i", "n_units",
               "first_unit", "head_len", "bc_off", "bc_len", "tagged", "status")
_PLAN = (2, FAKE, 1000, FAKE, FAKE, 1000, FAKE, FAKE, 500, FAKE, 4, 0, FAKE, FAKE, FAKE, FAKE, FAKE)
_WRITE_NAMES = ("mode", "text1", "n1_bytes", "line_start1", "text2", "n2_bytes", "line_start2", "text_i", "n_i_bytes", "n_units", "head_len",
                "bc_off", "bc_len", "tagged", "kept", "dst1", "dst2", "n_kept", "out1", "out1_bytes", "out2", "out2_bytes", "white_list",
                "white_list_bytes")
_WRITE = (2, FAKE, 1000, FAKE, FAKE, 1000, FAKE, FAKE, 500, 4, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 3, FAKE, 2000, FAKE, 2000, FAKE, 76)


def _with(good, names, **kw):
    assert set(kw) <= set(names)
    return tuple(kw.get(n, v) for n, v in zip(names, good))


def _plan(**kw):
    return _with(_PLAN, _PLAN_NAMES, **kw)


def _write(**kw):
    return _with(_WRITE, _WRITE_NAMES, **kw)


def _call(name, *args):
    L = _lib.load()
    rc = getattr(L, name)(*args)
    return rc, L.pg_last_error().decode()


_STLFR = {"mode": 1, "text_i": None, "n_i_bytes": 0}


@pytest.mark.parametrize("args,text", [
    (_plan(mode=0), "pg_fastq_prep_plan: mode 0 is neither PG_PREP_STLFR nor PG_PREP_TELLSEQ"),
    (_plan(mode=3), "pg_fastq_prep_plan: mode 3 is neither PG_PREP_STLFR nor PG_PREP_TELLSEQ"),
    (_plan(text1=None), "pg_fastq_prep_plan: text1 is null"),
    (_plan(text2=None), "pg_fastq_prep_plan: text2 is null"),
    (_plan(text_i=None), "pg_fastq_prep_plan: text_i is null"),
    (_plan(line_start1=None), "pg_fastq_prep_plan: line_start1 is null"),
    (_plan(line_start2=None), "pg_fastq_prep_plan: line_start2 is null"),
    (_plan(line_start_i=None), "pg_fastq_prep_plan: line_start_i is null"),
    (_plan(mode=1), "pg_fastq_prep_plan: text_i and line_start_i go with PG_PREP_TELLSEQ only"),
    (_plan(n1_bytes=-1), "pg_fastq_prep_plan: n1_bytes is negative (-1)"),
    (_plan(n2_bytes=-2), "pg_fastq_prep_plan: n2_bytes is negative (-2)"),
    (_plan(n_i_bytes=-3), "pg_fastq_prep_plan: n_i_bytes is negative (-3)"),
    (_plan(text1=FAKE + 8), "pg_fastq_prep_plan: text1 is not 16-byte aligned"),
    (_plan(text2=FAKE + 1), "pg_fastq_prep_plan: text2 is not 16-byte aligned"),
    (_plan(text_i=FAKE + 4), "pg_fastq_prep_plan: text_i is not 16-byte aligned"),
    (_plan(n_units=-3), "pg_fastq_prep_plan: n_units is negative (-3)"),
    (_plan(n_units=(1 << 40) + 1), "pg_fastq_prep_plan: n_units 1099511627777 beyond 2^40"),
    (_plan(first_unit=-1), "pg_fastq_prep_plan: first_unit -1 outside [0, 2^40]"),
    (_plan(head_len=None), "pg_fastq_prep_plan: head_len is null"),
    (_plan(bc_off=None), "pg_fastq_prep_plan: bc_off is null"),
    (_plan(bc_len=None), "pg_fastq_prep_plan: bc_len is null"),
    (_plan(tagged=None), "pg_fastq_prep_plan: tagged is null"),
    (_plan(status=None), "pg_fastq_prep_plan: status is null"),
])
def test_prep_plan_refusals(args, text):
    rc, msg = _call("pg_fastq_prep_plan", *args, None)
    assert rc == EINVAL and msg == text


@pytest.mark.parametrize("args,text", [
    (_write(mode=7), "pg_fastq_prep_write: mode 7 is neither PG_PREP_STLFR nor PG_PREP_TELLSEQ"),
    (_write(text1=None), "pg_fastq_prep_write: text1 is null"),
    (_write(text2=None), "pg_fastq_prep_write: text2 is null"),
    (_write(text_i=None), "pg_fastq_prep_write: text_i is null"),
    (_write(mode=1), "pg_fastq_prep_write: text_i and line_start_i go with PG_PREP_TELLSEQ only"),
    (_write(line_start1=None), "pg_fastq_prep_write: line_start1 is null"),
    (_write(line_start2=None), "pg_fastq_prep_write: line_start2 is null"),
    (_write(n1_bytes=-1), "pg_fastq_prep_write: n1_bytes is negative (-1)"),
    (_write(text2=FAKE + 2), "pg_fastq_prep_write: text2 is not 16-byte aligned"),
    (_write(n_units=-1), "pg_fastq_prep_write: n_units is negative (-1)"),
    (_write(head_len=None), "pg_fastq_prep_write: head_len is null"),
    (_write(bc_off=None), "pg_fastq_prep_write: bc_off is null"),
    (_write(bc_len=None), "pg_fastq_prep_write: bc_len is null"),
    (_write(tagged=None), "pg_fastq_prep_write: tagged is null"),
    (_write(dst1=None), "pg_fastq_prep_write: dst1 is null"),
    (_write(dst2=None), "pg_fastq_prep_write: dst2 is null"),
    (_write(out1=None), "pg_fastq_prep_write: out1 is null"),
    (_write(out2=None), "pg_fastq_prep_write: out2 is null"),
    (_write(out1_bytes=-1), "pg_fastq_prep_write: out1_bytes is negative (-1)"),
    (_write(out2_bytes=-5), "pg_fastq_prep_write: out2_bytes is negative (-5)"),
    (_write(white_list_bytes=-1), "pg_fastq_prep_write: white_list_bytes is negative (-1)"),
    (_write(**_STLFR), "pg_fastq_prep_write: white_list goes with PG_PREP_TELLSEQ only"),
    (_write(n_kept=-1), "pg_fastq_prep_write: n_kept -1 outside [0, n_units = 4]"),
    (_write(n_kept=5), "pg_fastq_prep_write: n_kept 5 outside [0, n_units = 4]"),
])
def test_prep_write_refusals(args, text):
    rc, msg = _call("pg_fastq_prep_write", *args, None)
    assert rc == EINVAL and msg == text


def test_nothing_to_do_is_ok_and_launches_nothing():
    # (no units: PG_OK before any HIP call; a null kept is "every unit", a null white list "none", not errors)
    assert _call("pg_fastq_prep_plan", *_plan(n_units=0), None)[0] == OK
    assert _call("pg_fastq_prep_plan", *_plan(n_units=0, line_start_i=None, **_STLFR), None)[0] == OK
    assert _call("pg_fastq_prep_write", *_write(n_kept=0, kept=None, white_list=None), None)[0] == OK
    assert _call("pg_fastq_prep_write", *_write(n_kept=0, n_units=0, white_list=None, **_STLFR), None)[0] == OK


def _prep(argv, capsys):
    rc = cli.main_preprocess_reads(argv)
    return rc, capsys.readouterr().err


def _sort(argv, capsys):
    rc = cli.main_sort_barcodes(argv)
    return rc, capsys.readouterr().err


def test_preprocess_reads_refuses_bad_arguments(tmp_path, capsys):
    f = str(tmp_path / "a.fq")
    open(f, "w").close()
    pre = str(tmp_path / "out")
    who = "preprocess_reads: "
    assert _prep(["--short_type", "tellseq", "-1", f, "-2", f, "-o", pre], capsys) == (1, who + "tellseq reads need their index reads: -I INDEX\n")
    assert _prep(["--short_type", "stlfr", "-1", f, "-2", f, "-I", f, "-o", pre], capsys) == (
        1, who + "-I INDEX goes with --short_type tellseq only, not with stlfr\n")
    assert _prep(["--short_type", "10x", "-1", f, "-2", f, "-o", pre], capsys) == (1, who + "--short_type must be one of stlfr, tellseq (got '10x')\n")
    assert _prep(["--short_type", "hybrid", "-1", f, "-2", f, "-o", pre], capsys) == (
        1, who + "--short_type must be one of stlfr, tellseq (got 'hybrid')\n")
    assert _prep(["--short_type", "stlfr", "-1", f, "-o", pre], capsys) == (1, who + "the raw reads are -1 R1 -2 R2 (both)\n")
    assert _prep(["--short_type", "stlfr", "-1", f, "-2", f, "-o", pre + ".gz"], capsys) == (
        1, who + f"{pre}.gz: the reads are written as plain text (PREFIX_1.fq, PREFIX_2.fq), gzip output is not supported\n")
    # an output that is one of the inputs
    same = str(tmp_path / "x_1.fq")
    open(same, "w").close()
    assert _prep(["--short_type", "stlfr", "-1", same, "-2", f, "-o", str(tmp_path / "x")], capsys) == (
        1, who + f"the outputs must differ from the inputs (got {os.path.realpath(same)})\n")
    wl = str(tmp_path / "y.wl")
    open(wl, "w").close()
    assert _prep(["--short_type", "tellseq", "-1", f, "-2", f, "-I", wl, "-o", str(tmp_path / "y")], capsys) == (
        1, who + f"the outputs must differ from the inputs (got {os.path.realpath(wl)})\n")
    missing = str(tmp_path / "none.fq")
    assert _prep(["--short_type", "stlfr", "-1", f, "-2", missing, "-o", pre], capsys) == (1, who + f"{missing}: no such file\n")
    assert sorted(os.listdir(tmp_path)) == ["a.fq", "x_1.fq", "y.wl"]            # nothing was written, and the inputs are what they were
    assert os.path.getsize(same) == 0
    with pytest.raises(SystemExit) as e:                     # (no --short_type at all: argparse's usage, exit status 1 as the other tools)
        cli.main_preprocess_reads(["-1", f, "-2", f, "-o", pre])
    assert e.value.code == 1
    capsys.readouterr()


def test_sort_barcodes_refuses_bad_short_type_arguments(tmp_path, capsys):
    f = str(tmp_path / "a.fq")
    open(f, "w").close()
    out = str(tmp_path / "o.fq")
    who = "sort_barcodes: "
    assert _sort(["--short_type", "tellseq", "-1", f, "-2", f, "-o", out], capsys) == (1, who + "tellseq reads need their index reads: -I INDEX\n")
    assert _sort(["-1", f, "-2", f, "-I", f, "-o", out], capsys) == (1, who + "-I INDEX goes with --short_type tellseq only, not with 10x\n")
    assert _sort(["--short_type", "stlfr", "-1", f, "-2", f, "-I", f, "-o", out], capsys) == (
        1, who + "-I INDEX goes with --short_type tellseq only, not with stlfr\n")
    assert _sort(["--short_type", "stlfr", "-i", f, "-o", out], capsys) == (1, who + "raw stlfr reads are given as -1 R1 -2 R2, not as -i\n")
    assert _sort(["--short_type", "tellseq", "-I", f, "-i", f, "-o", out], capsys) == (1, who + "raw tellseq reads are given as -1 R1 -2 R2, not as -i\n")
    assert _sort(["--short_type", "pacbio", "-1", f, "-2", f, "-o", out], capsys) == (
        1, who + "--short_type must be one of 10x, stlfr, tellseq (got 'pacbio')\n")
    assert _sort(["--check", "--short_type", "tellseq", "-1", f, "-2", f], capsys) == (2, who + "tellseq reads need their index reads: -I INDEX\n")
    assert _sort(["--short_type", "stlfr", "-1", f, "-2", f, "-o", f], capsys) == (1, who + f"the output must differ from the inputs (got {f})\n")
    index = str(tmp_path / "i.fq")
    open(index, "w").close()
    assert _sort(["--short_type", "tellseq", "-1", f, "-2", f, "-I", index, "-o", index], capsys) == (
        1, who + f"the output must differ from the inputs (got {index})\n")
    assert _sort(["--short_type", "stlfr", "-1", f, "-2", f, "-o", out + ".gz"], capsys) == (
        1, who + f"{out}.gz: the sorted reads are written as plain text, gzip output is not supported\n")
    missing = str(tmp_path / "none.fq")
    assert _sort(["--short_type", "tellseq", "-1", f, "-2", f, "-I", missing, "-o", out], capsys) == (1, who + f"{missing}: no such file\n")
    assert not os.path.exists(out) and os.path.getsize(f) == 0


def test_orchestrator_refuses_bad_short_type_arguments(tmp_path, capsys):
    from pangaea_amd import pangaea
    f = str(tmp_path / "a.fq")
    base = ["-o", str(tmp_path / "out"), "--sort_reads"]
    for argv, text in ((["-1", f, "-2", f, "--short_type", "tellseq"], "tellseq reads need their index reads: -I INDEX"),
                       (["-1", f, "-2", f, "--index", f], "-I INDEX goes with --short_type tellseq only, not with 10x"),
                       (["-i", f, "--short_type", "stlfr"], "raw stlfr reads are given as -1 R1 -2 R2, not as -i"),
                       (["-1", f, "-2", f, "--short_type", "nanopore"], "--short_type must be one of 10x, stlfr, tellseq (got 'nanopore')")):
        with pytest.raises(SystemExit) as e:
            pangaea.main(base + argv)
        assert e.value.code == 2 and text in capsys.readouterr().err
    with pytest.raises(SystemExit):
        pangaea.main(["-o", str(tmp_path / "out"), "-1", f, "-2", f, "--short_type", "stlfr"])
    assert "they are prepared and sorted by --sort_reads" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "out")
