"""Raw stLFR and TELL-seq read pairs brought to the BX:Z: form on the GPU (pangaea_amd/prepreads.py; pg_fastq_prep_plan,
pg_fastq_prep_write; sortreads.sort_fastq / check_fastq with ``short_type``) against the plain-Python restatement of the rules in
tests/_prep_ref.py, which tests/test_prep_reads_host.py holds against the reference's own binaries.  Every comparison is exact:
bytes and integers."""
import gzip
import json
import os
import random

import pytest
import torch

from pangaea_amd import _lib, cli, prepreads, sortreads, synth

from . import _prep_ref as ref
from . import _sort_ref
from .conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CLEAN = [[0, -1]] * 3            # the status rows of texts without a malformed record (PG_FASTQ_CLEAN as int64)
PREP = os.path.join(GOLDEN, "prep")
FORMAT = _lib.STATUS_FASTQ_FORMAT


def _rec(header: bytes, seq: bytes = b"ACGTTGCA", third: bytes = b"+", eol: bytes = b"\n") -> bytes:
    return header + b"\n" + seq + eol + third + eol + b"I" * len(seq) + eol


def _on_device(data: bytes) -> torch.Tensor:
    return torch.frombuffer(bytearray(data + b"\0" * 32), dtype=torch.uint8).to(DEV)


def _plan_of(short_type: str, r1: bytes, r2: bytes, i1: bytes | None = None, first_unit: int = 0):
    datas = [r1, r2] + ([i1] if short_type == "tellseq" else [])
    texts = [_on_device(d) for d in datas]
    idxs, lines = zip(*(sortreads.line_index(t, len(d)) for t, d in zip(texts, datas)))
    assert len(set(lines)) == 1 and lines[0] % 4 == 0
    return prepreads.Plan(_lib.PREP_MODES[short_type], texts, [len(d) for d in datas], list(idxs), lines[0] // 4, first_unit)


def _expected_plan(short_type: str, r1: bytes, r2: bytes, i1: bytes | None = None, first_unit: int = 0) -> tuple:
    """(head_len, bc_off, bc_len, tagged, status rows) as pg_fastq_prep_plan states them, unit by unit from the restatement: a
    malformed unit leaves 0, -1, 0, 0 and its file's row keeps the smallest ordinal"""
    n_files = 3 if short_type == "tellseq" else 2
    files = [ref.records_of(d) for d in (r1, r2, i1)[:n_files]]
    starts = []                                              # the byte offset of every line of R1 / of I1
    for d in (r1, i1 if short_type == "tellseq" else None):
        at, offs = 0, []
        for line in ref.contents_of(d or b""):
            offs.append(at)
            at += len(line) + 1
        starts.append(offs)
    rows = [[0, -1] for _ in range(3)]
    out = ([], [], [], [])
    for u in range(len(files[0])):
        marks = [(f, ref.NO_AT if not rec[u][0].startswith(b"@") else ref.NO_PLUS) for f, rec in enumerate(files)
                 if not rec[u][0].startswith(b"@") or not rec[u][2].startswith(b"+")]
        bad = list(marks)
        vals = (0, -1, 0, 0)
        if not marks:
            h = files[0][u][0]
            try:
                if short_type == "stlfr":
                    p, B, tag = ref.stlfr_plan(h)
                    vals = (p, starts[0][4 * u] + p + 1, len(B), int(tag))
                else:
                    s, B, tag = ref.tellseq_plan(h, files[2][u][1])
                    vals = (s, starts[1][4 * u + 1], len(B), int(tag))
            except ref.Malformed as e:
                bad = [(0, e.reason)]
        for f, reason in bad:
            if rows[f][1] == -1:
                rows[f] = [FORMAT, (first_unit + u) << 8 | reason]
        for o, v in zip(out, vals):
            o.append(v)
    return (*out, rows)


def _assert_plan(short_type: str, r1: bytes, r2: bytes, i1: bytes | None = None, first_unit: int = 0):
    plan = _plan_of(short_type, r1, r2, i1, first_unit)
    head, off, length, tagged, rows = _expected_plan(short_type, r1, r2, i1, first_unit)
    assert plan.head_len.cpu().tolist() == head
    assert plan.bc_off.cpu().tolist() == off
    assert plan.bc_len.cpu().tolist() == length
    assert plan.tagged.cpu().tolist() == tagged
    assert plan.status.cpu().tolist() == rows
    return plan, rows


def _padded(h: bytes, total: int) -> bytes:
    """``h`` as a header of exactly ``total`` bytes: text behind a space added, or the end cut off"""
    return (h + b" " + b"y" * total)[:total]


def _straddling_stlfr_headers() -> list:
    """headers of exactly 64, 65, 128 and 200 bytes with '#', '/', the first and the second '_' at bytes 58 .. 68: every alignment
    of each question across the 64-byte turn, the byte behind '#' and behind the first '_' (the zero tests) in the next turn
    included; where the header ends before the barcode is complete the unit is malformed, and expected to be"""
    out = []
    for total in (64, 65, 128, 200):
        for pos in range(58, 69):
            x = b"@" + b"x" * 80
            for B in (b"0_5_1", b"5_0_1", b"7_8_0"):                                             # '#' at pos
                out.append(_padded(x[:pos] + b"#" + B + b"/1", total))
            out.append(_padded(x[:pos - 9] + b"#1_2_3456/1", total))                             # '/' at pos
            for f1 in (b"0", b"7"):
                for f2 in (b"0", b"6"):
                    out.append(_padded(x[:pos - 2] + b"#" + f1 + b"_" + f2 + b"_6/1", total))    # the first '_' at pos
            for f2 in (b"0", b"5"):
                out.append(_padded(x[:pos - 4] + b"#1_" + f2 + b"_9/1", total))                  # the second '_' at pos
    assert all(len(h) in (64, 65, 128, 200) for h in out)
    return out


STLFR_HEADERS = [b"@f#" + f1 + b"_" + f2 + b"_9/1" for f1 in (b"0", b"00", b"0x", b"10", b"") for f2 in (b"0", b"00", b"0x", b"10", b"")] + [
    b"@more#1_2_3_4_5/1",                                    # more '_' in f3
    b"@more#0_2_3_4_5/1", b"@more#1_0_3_0_0/1", b"@more#1_2_0_0_0/1",
    b"@two#hashes#7_8_9/1",                                  # a '#' inside the read name: the first wins
    b"@two#0_1#2_3/1", b"@two#1_0_#2/1",
    b"@a/b#1_2_3/1",                                         # a '/' in front of the '#' cuts nothing
    b"@a_b_c#1_2_3/1",                                       # '_' in front of the '#' count for nothing
    b"@nos#12_34_56",                                        # no '/': the barcode goes to the end
    b"@nos#12_34_",                                          # an empty third field
    b"@behind#1_2_3/1 text_behind/the#slash",
    b"@behind#1_2_3/_/", b"@cr#1_2_3\r",                     # ('\r' is an ordinary byte: part of f3 here)
    b"@x#1_2_" + b"3" * 249,                                 # 253 bytes: the longest barcode
    b"@" + b"n" * 300 + b"#11_22_33/1",                      # five turns until the '#'
    b"@" + b"n" * 126 + b"#0_22_33/1 " + b"t" * 100,
] + _straddling_stlfr_headers()


def test_plan_of_hand_built_stlfr_headers():
    r1 = b"".join(_rec(h) for h in STLFR_HEADERS)
    r2 = b"".join(_rec(b"@mate%d#9_9_9/2" % i, b"TTGACC") for i in range(len(STLFR_HEADERS)))
    head, off, length, tagged, rows = _expected_plan("stlfr", r1, r2)
    assert sum(tagged) >= 150 and sum(1 for t, o in zip(tagged, off) if not t and o >= 0) >= 100 and off.count(-1) >= 10     # (all kinds)
    _assert_plan("stlfr", r1, r2)
    # the well-formed ones alone: clean status rows; and without the text's final newline
    good = [h for h, o in zip(STLFR_HEADERS, off) if o >= 0]
    r1 = b"".join(_rec(h) for h in good)
    r2 = b"".join(_rec(b"@m", b"TT") for _ in good)
    for a, b in ((r1, r2), (r1[:-1], r2[:-1])):
        _, rows = _assert_plan("stlfr", a, b)
        assert rows == CLEAN


def test_plan_of_hand_built_tellseq_units():
    x = b"@" + b"x" * 300
    heads = [x[:63] + b" s63", x[:64] + b" s64", x[:65] + b" s65", x[:62] + b"  two", b"@tab\tbefore the space", b"@tab\tonly", b"@nospace",
             x[:64], x[:65], x[:200], x[:150] + b" far", x[:127] + b" 127", x[:128] + b" 128", b"@a b", b"@ x", b"@\r x"]
    index = [b"", b"A" * 17, b"ACGTACGTACGTACGTAC", b"C" * 19, b"G" * 18 + b"\r", b"ACGTNNGTACGTACGTAC", b"T" * 18, b"A" * 200]
    units = [(h, index[(i + j) % len(index)]) for j in range(3) for i, h in enumerate(heads)]
    r1 = b"".join(_rec(h, b"ACGT" * (1 + i % 5), b"+" + h[1:] if i % 4 == 0 else b"+") for i, (h, _) in enumerate(units))
    r2 = b"".join(_rec(b"@m%d 2:N" % i, b"TTGACC") for i in range(len(units)))
    i1 = b"".join(_rec(b"@i%d" % i, b) for i, (_, b) in enumerate(units))
    head, off, length, tagged, rows = _expected_plan("tellseq", r1, r2, i1)
    assert rows == CLEAN and 10 <= sum(tagged) < len(units) and set(length) == {0, 17, 18, 19, 200}
    _assert_plan("tellseq", r1, r2, i1)
    _assert_plan("tellseq", r1[:-1], r2, i1[:-1])


def test_plan_status_words():
    ok1 = [b"@r%d#1_2_%d/1" % (i, i) for i in range(9)]
    long_ok, too_long = b"@l#1_2_" + b"3" * 249, b"@l#1_2_" + b"3" * 250
    assert len(long_ok) - 3 == 253

    def stlfr(h1, h2=None, thirds=(b"+", b"+"), first_unit=0):
        r1 = b"".join(_rec(h, third=thirds[0] if isinstance(thirds[0], bytes) else thirds[0][i]) for i, h in enumerate(h1))
        r2 = b"".join(_rec(h, third=thirds[1] if isinstance(thirds[1], bytes) else thirds[1][i]) for i, h in enumerate(h2 or [b"@m"] * len(h1)))
        return _assert_plan("stlfr", r1, r2, first_unit=first_unit)[1]

    def with_at(items, at, value):
        return [value if i == at else x for i, x in enumerate(items)]

    assert stlfr(ok1 + [long_ok]) == CLEAN
    for at in (4, 8):                                        # a middle unit, and the last
        for bad, reason in ((b"@nohash", ref.NO_HASH), (b"@one#1_2", ref.FEW_FIELDS), (b"@none#12", ref.FEW_FIELDS), (b"@cut#12/1_2_3", ref.FEW_FIELDS),
                            (b"@empty#/1_2_3", ref.FEW_FIELDS), (too_long, ref.LONG_TAG), (b"r#1_2_3", ref.NO_AT)):
            assert stlfr(with_at(ok1, at, bad)) == [[FORMAT, at << 8 | reason], [0, -1], [0, -1]]
        assert stlfr(ok1, with_at([b"@m"] * 9, at, b"m")) == [[0, -1], [FORMAT, at << 8 | ref.NO_AT], [0, -1]]
        plus = with_at([b"+"] * 9, at, b"-")
        assert stlfr(ok1, thirds=(plus, b"+")) == [[FORMAT, at << 8 | ref.NO_PLUS], [0, -1], [0, -1]]
        assert stlfr(ok1, thirds=(b"+", plus)) == [[0, -1], [FORMAT, at << 8 | ref.NO_PLUS], [0, -1]]
    # the smallest ordinal wins, in every file of its own; '@' is asked before '+', both before the barcode
    assert stlfr(with_at(with_at(ok1, 6, b"@nohash"), 2, b"@few#1_2")) == [[FORMAT, 2 << 8 | ref.FEW_FIELDS], [0, -1], [0, -1]]
    assert stlfr(with_at(with_at(ok1, 7, b"@few#1_2"), 3, too_long), with_at([b"@m"] * 9, 5, b"m")) == [
        [FORMAT, 3 << 8 | ref.LONG_TAG], [FORMAT, 5 << 8 | ref.NO_AT], [0, -1]]
    assert stlfr(with_at(ok1, 1, b"nohash"), thirds=(with_at([b"+"] * 9, 1, b"x"), b"+")) == [[FORMAT, 1 << 8 | ref.NO_AT], [0, -1], [0, -1]]
    # ordinals count from first_unit on (pieces)
    assert stlfr(with_at(ok1, 4, b"@nohash"), first_unit=1_000_000_000_000) == [[FORMAT, 1_000_000_000_004 << 8 | ref.NO_HASH], [0, -1], [0, -1]]
    # TELL-seq: the third file has a row of its own; a barcode of any length is no error
    heads = [b"@t%d 1:N" % i for i in range(6)]
    r1, r2 = b"".join(_rec(h) for h in heads), b"".join(_rec(h, b"TT") for h in heads)
    for at in (2, 5):
        i1 = b"".join(_rec(b"i%d" % i if i == at else b"@i%d" % i, b"A" * 18) for i in range(6))
        assert _assert_plan("tellseq", r1, r2, i1)[1] == [[0, -1], [0, -1], [FORMAT, at << 8 | ref.NO_AT]]
        i1 = b"".join(_rec(b"@i%d" % i, b"A" * (300 if i == at else 18), b"=" if i == at else b"+") for i in range(6))
        assert _assert_plan("tellseq", r1, r2, i1)[1] == [[0, -1], [0, -1], [FORMAT, at << 8 | ref.NO_PLUS]]
    i1 = b"".join(_rec(b"@i%d" % i, b"A" * 300) for i in range(6))
    assert _assert_plan("tellseq", r1, r2, i1)[1] == CLEAN


def test_plan_with_an_index_that_is_none_reads_nothing_and_says_so():
    heads = [b"@r%d#1_2_3/1" % i for i in range(8)]
    r1, r2 = b"".join(_rec(h) for h in heads), b"".join(_rec(h, b"TT") for h in heads)
    plan = _plan_of("stlfr", r1, r2)
    # (file, entry of its line index, the value put there, the unit that is hit)
    for file, entry, value, unit in ((0, 13, -7, 3), (0, 14, 1 << 50, 3), (1, 4 * 8, len(r2) + 1, 7), (1, 5, 0, 1)):
        idxs = [ix.clone() for ix in plan.idxs]
        idxs[file][entry] = value
        got = prepreads.Plan(plan.mode, plan.texts, plan.sizes, idxs, 8)
        rows = got.status.cpu().tolist()
        assert rows[1 - file] == [0, -1] and rows[2] == [0, -1] and rows[file] == [FORMAT, unit << 8 | _lib.FASTQ_BAD_INDEX]
        assert got.tagged.cpu().tolist() == [int(u != unit) for u in range(8)]
        assert got.bc_off.cpu().tolist() == [-1 if u == unit else o for u, o in enumerate(plan.bc_off.cpu().tolist())]


def _written(short_type: str, r1: bytes, r2: bytes, i1: bytes | None = None) -> dict:
    """the two-file form, the white list and the interleaved form, as the kernels write them"""
    plan = _plan_of(short_type, r1, r2, i1)
    assert plan.status.cpu().tolist() == CLEAN
    kept = plan.kept()
    len1, len2 = plan.record_bytes(kept)
    n1, n2, n_kept = int(len1.sum()), int(len2.sum()), int(len1.numel())
    guard = 64                                               # bytes behind each output that must stay as they were
    out1 = torch.full((n1 + guard,), 0xEE, dtype=torch.uint8, device=DEV)
    out2 = torch.full((n2 + guard,), 0xEE, dtype=torch.uint8, device=DEV)
    wl = torch.full((19 * n_kept + guard,), 0xEE, dtype=torch.uint8, device=DEV) if short_type == "tellseq" else None
    plan.write(kept, torch.cumsum(len1, 0) - len1, torch.cumsum(len2, 0) - len2, out1, n1, out2, n2, wl[:19 * n_kept] if wl is not None else None)
    for buf, n in ((out1, n1), (out2, n2)) + (((wl, 19 * n_kept),) if wl is not None else ()):
        assert buf[n:].cpu().tolist() == [0xEE] * guard
    text, n, units = prepreads.interleaved_text(plan)
    assert units == n_kept and n == n1 + n2
    return {"out1": bytes(out1[:n1].cpu().numpy()), "out2": bytes(out2[:n2].cpu().numpy()),
            "wl": bytes(wl[:19 * n_kept].cpu().numpy()) if wl is not None else None, "interleaved": bytes(text[:n].cpu().numpy()),
            "tagged": int(plan.tagged.sum())}


def _assert_written(short_type: str, r1: bytes, r2: bytes, i1: bytes | None = None) -> dict:
    want = ref.preprocess(short_type, r1, r2, i1)
    got = _written(short_type, r1, r2, i1)
    assert got["out1"] == want["out1"] and got["out2"] == want["out2"] and got["wl"] == want["wl"]
    assert got["interleaved"] == ref.interleaved(want) and got["tagged"] == want["tagged"]
    return want


def _random_units(rng: random.Random, short_type: str, n: int, lengths=(0, 1, 150)) -> tuple:
    r1, r2, i1 = [], [], []
    for i in range(n):
        L1, L2 = rng.choice(lengths), rng.choice(lengths)
        if i == n - 1:                                       # (the last quality lines are not empty: the final newline can be cut off)
            L1, L2 = max(L1, 1), max(L2, 1)
        eol = b"\r\n" if rng.random() < 0.1 else b"\n"
        seq1, seq2 = (bytes(rng.choice(b"ACGTN") for _ in range(L)) for L in (L1, L2))
        name = b"@V%d" % rng.randrange(10 ** rng.randrange(1, 60))
        if short_type == "stlfr":
            fields = [rng.choice([b"0", b"0", b"%d" % rng.randrange(1, 1537), b"00", b""]) for _ in range(3)]
            if rng.random() < 0.5:
                fields = [b"%d" % rng.randrange(1, 1537) for _ in range(3)]
            tail = rng.choice([b"/1", b"", b"/1 extra", b"/1\tBX:Z:old-1"])
            h1 = name + b"#" + b"_".join(fields) + tail
            h2 = name + b"#" + b"_".join(fields) + b"/2"
        else:
            h1 = name + rng.choice([b" 1:N:0:ACGT", b"", b"\tx y", b" "])
            h2 = name + b" 2:N:0:ACGT"
            b = bytes(rng.choice(b"ACGTN") for _ in range(rng.choice([18] * 6 + [0, 17, 19, 36])))
            i1.append(_rec(name + b" 1:N:0", b + (b"\r" if rng.random() < 0.05 else b"")))
        third = rng.choice([b"+", b"+", b"+" + h1[1:]])
        r1.append(_rec(h1, seq1, third, eol))
        r2.append(_rec(h2, seq2, b"+", eol))
    return b"".join(r1), b"".join(r2), b"".join(i1) if short_type == "tellseq" else None


@pytest.mark.parametrize("short_type", ["stlfr", "tellseq"])
def test_written_text_equals_the_restatement(short_type):
    rng = random.Random(20240 + len(short_type))
    for n in (1, 2, 63, 64, 65, 1000):
        r1, r2, i1 = _random_units(rng, short_type, n)
        want = _assert_written(short_type, r1, r2, i1)
        assert want["pairs"] == n
        if n == 65:                                          # a last line without '\n', in one file and in all
            _assert_written(short_type, r1[:-1], r2, i1)
            _assert_written(short_type, r1[:-1], r2[:-1], i1[:-1] if i1 else None)
    # reads of 5 000 bases beside empty ones
    r1, r2, i1 = _random_units(rng, short_type, 12, lengths=(0, 1, 5000))
    _assert_written(short_type, r1, r2, i1)


def test_write_skips_what_the_plan_arrays_do_not_allow():
    """whatever the device arrays hold, nothing outside the outputs is written: a unit whose plan, order or place is none of
    this text's is left out, its neighbours are written"""
    rng = random.Random(7)
    r1, r2, _ = _random_units(rng, "stlfr", 40, lengths=(30,))
    r1 = r1.replace(b"\r", b"")
    r2 = r2.replace(b"\r", b"")
    want = ref.preprocess("stlfr", r1, r2)
    plan = _plan_of("stlfr", r1, r2)
    len1, len2 = plan.record_bytes(None)
    n1, n2 = int(len1.sum()), int(len2.sum())
    at1, at2 = torch.cumsum(len1, 0) - len1, torch.cumsum(len2, 0) - len2
    tagged = plan.tagged.nonzero().flatten().cpu().tolist()
    t0, t1 = tagged[0], tagged[-1]

    def run(spoil) -> tuple:
        p = _plan_of("stlfr", r1, r2)
        d1, d2, kept = at1.clone(), at2.clone(), torch.arange(40, dtype=torch.int64, device=DEV)
        skipped = spoil(p, d1, d2, kept)
        out1 = torch.full((n1 + 64,), 0xEE, dtype=torch.uint8, device=DEV)
        out2 = torch.full((n2 + 64,), 0xEE, dtype=torch.uint8, device=DEV)
        p.write(kept, d1, d2, out1, n1, out2, n2)
        torch.cuda.synchronize()
        for out, units, at in ((out1, want["units1"], at1.cpu().tolist()), (out2, want["units2"], at2.cpu().tolist())):
            got = bytes(out.cpu().numpy())
            assert got[-64:] == b"\xee" * 64
            for u, rec in enumerate(units):
                assert got[at[u]:at[u] + len(rec)] == (b"\xee" * len(rec) if u in skipped else rec), u
        return skipped

    def set_(t, i, v):
        t[i] = v

    assert run(lambda p, d1, d2, k: set()) == set()
    run(lambda p, d1, d2, k: set_(p.head_len, 3, 1 << 40) or {3})
    run(lambda p, d1, d2, k: set_(p.head_len, 5, -1) or {5})
    run(lambda p, d1, d2, k: set_(p.bc_off, t0, -5) or {t0})
    run(lambda p, d1, d2, k: set_(p.bc_off, t1, len(r1) - 2) or {t1})
    run(lambda p, d1, d2, k: set_(p.bc_len, t0, 254) or {t0})
    run(lambda p, d1, d2, k: set_(p.bc_len, t0, -3) or {t0})
    run(lambda p, d1, d2, k: set_(k, 7, 40) or {7})
    run(lambda p, d1, d2, k: set_(k, 9, -1) or {9})
    run(lambda p, d1, d2, k: set_(d1, 39, n1 - 3) or {39})
    run(lambda p, d1, d2, k: set_(d2, 0, -1) or {0})
    run(lambda p, d1, d2, k: set_(d2, 11, 1 << 45) or {11})
    run(lambda p, d1, d2, k: set_(p.idxs[0], 4 * 6 + 2, 0) or {6})
    run(lambda p, d1, d2, k: set_(p.idxs[1], 4 * 40, len(r2) + 9) or {39})


def _files(tmp_path, **datas) -> dict:
    paths = {}
    for name, data in datas.items():
        paths[name] = str(tmp_path / (name + ".fq"))
        with open(paths[name], "wb") as f:
            f.write(data)
    return paths


def _read(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def test_goldens_through_preprocess_reads(tmp_path):
    g = lambda name: os.path.join(PREP, name)                # noqa: E731
    for suffix in ("", ".gz"):
        pre = str(tmp_path / ("s" + suffix.strip(".")))
        res = prepreads.preprocess_reads("stlfr", g("stlfr_R1.fq" + suffix), g("stlfr_R2.fq" + suffix), pre)
        assert _read(pre + "_1.fq") == _read(g("stlfr.ref_1.fq")) and _read(pre + "_2.fq") == _read(g("stlfr.ref_2.fq"))
        assert (res["short_type"], res["pairs"], res["tagged_pairs"], res["untagged_pairs"]) == ("stlfr", 15, 9, 6)
        assert res["bytes"] == os.path.getsize(pre + "_1.fq") + os.path.getsize(pre + "_2.fq") and res["files"] == [pre + "_1.fq", pre + "_2.fq"]
        assert set(res["device_ms"]) == {"index", "plan", "write"} and not os.path.exists(pre + ".wl")
    # TELL-seq: plain, and from gzip copies made here; through the command line
    srcs = {n: g("tellseq_" + n + ".fq") for n in ("R1", "R2", "I1")}
    packed = {}
    for n, p in srcs.items():
        packed[n] = str(tmp_path / (n + ".fq.gz"))
        with gzip.open(packed[n], "wb") as z:
            z.write(_read(p))
    for k, files in enumerate((srcs, packed)):
        pre = str(tmp_path / ("t%d" % k))
        res = prepreads.preprocess_reads("tellseq", files["R1"], files["R2"], pre, index=files["I1"])
        assert _read(pre + "_1.fq") == _read(g("tellseq.ref_1.fq")) and _read(pre + "_2.fq") == _read(g("tellseq.ref_2.fq"))
        assert _read(pre + ".wl") == _read(g("tellseq.ref.wl"))
        assert (res["pairs"], res["kept_pairs"], res["dropped_pairs"]) == (10, 6, 4)
        assert res["bytes"] == sum(os.path.getsize(pre + s) for s in ("_1.fq", "_2.fq", ".wl"))
    assert sorted(os.listdir(tmp_path)) == sorted(["s_1.fq", "s_2.fq", "sgz_1.fq", "sgz_2.fq", "R1.fq.gz", "R2.fq.gz", "I1.fq.gz"]
                                                   + ["t%d%s" % (k, s) for k in (0, 1) for s in ("_1.fq", "_2.fq", ".wl")])


def test_preprocess_reads_command(tmp_path, capsys):
    g = lambda name: os.path.join(PREP, name)                # noqa: E731
    pre = str(tmp_path / "c")
    assert cli.main_preprocess_reads(["--short_type", "tellseq", "-1", g("tellseq_R1.fq"), "-2", g("tellseq_R2.fq"), "-I", g("tellseq_I1.fq"), "-o", pre]) == 0
    res = json.loads(capsys.readouterr().out)
    assert (res["pairs"], res["kept_pairs"], res["dropped_pairs"]) == (10, 6, 4) and _read(pre + ".wl") == _read(g("tellseq.ref.wl"))
    assert _read(pre + "_1.fq") == _read(g("tellseq.ref_1.fq")) and _read(pre + "_2.fq") == _read(g("tellseq.ref_2.fq"))
    # a malformed record: status 1, the message names file and record, and nothing is left behind
    p = _files(tmp_path, r1=_rec(b"@a#1_2_3/1") + _rec(b"@b#1_2/1"), r2=_rec(b"@a") * 2, good=_rec(b"@a#1_2_3/1") * 2, short=_rec(b"@a"),
               cut=_rec(b"@a") + b"@b\nAC\n")
    bad = str(tmp_path / "bad")
    assert cli.main_preprocess_reads(["--short_type", "stlfr", "-1", p["r1"], "-2", p["r2"], "-o", bad]) == 1
    assert capsys.readouterr().err == f"preprocess_reads: {p['r1']}: record 1: its stLFR barcode holds fewer than two '_' (PG_EFORMAT)\n"
    assert cli.main_preprocess_reads(["--short_type", "stlfr", "-1", p["good"], "-2", p["short"], "-o", bad]) == 1
    assert capsys.readouterr().err == (f"preprocess_reads: {p['short']} ends after 1 records, {p['good']} holds more: "
                                       "the read files must have the same number of records (PG_EFORMAT)\n")
    assert cli.main_preprocess_reads(["--short_type", "stlfr", "-1", p["good"], "-2", p["cut"], "-o", bad]) == 1
    assert capsys.readouterr().err == f"preprocess_reads: {p['cut']}: record 1: the file ends inside it (2 of its 4 lines) (PG_EFORMAT)\n"
    assert [f for f in os.listdir(tmp_path) if f.startswith("bad")] == []


@pytest.mark.parametrize("short_type", ["stlfr", "tellseq"])
def test_pieces_give_the_one_piece_output(short_type, tmp_path, monkeypatch):
    rng = random.Random(99)
    # records of different byte lengths in R1, R2 and I1: the piece boundaries fall at different ordinals in each file
    r1, r2, i1 = _random_units(rng, short_type, 300, lengths=(150, 151, 40))
    r2 = r2.replace(b" 2:N:0:ACGT", b"")
    want = ref.preprocess(short_type, r1, r2, i1)
    p = _files(tmp_path, r1=r1[:-1], r2=r2, **({"i1": i1} if i1 else {}))
    assert len(r1) > 10 * 4096 and len(r2) > 8 * 4096 and len(r1) - len(r2) > 4096 and (i1 is None or len(i1) < len(r2) // 2)
    outs = []
    for piece in (None, "4096"):
        if piece:
            monkeypatch.setenv("PG_FILTER_PIECE_BYTES", piece)
        pre = str(tmp_path / ("p" + (piece or "one")))
        res = prepreads.preprocess_reads(short_type, p["r1"], p["r2"], pre, index=p.get("i1"))
        outs.append([_read(pre + s) for s in ("_1.fq", "_2.fq") + ((".wl",) if i1 else ())])
        assert res["pairs"] == 300 and res.get("tagged_pairs", res.get("kept_pairs")) == want["tagged"]
    assert outs[0] == outs[1] == [want["out1"], want["out2"]] + ([want["wl"]] if i1 else [])
    # a malformed record in a late piece is named by its ordinal in the file
    lines = r1.split(b"\n")
    lines[4 * 250] = b"@nohash" if short_type == "stlfr" else b"nomark"
    with open(p["r1"], "wb") as f:
        f.write(b"\n".join(lines))
    with pytest.raises(ValueError, match=r"r1\.fq: record 250: "):
        prepreads.preprocess_reads(short_type, p["r1"], p["r2"], str(tmp_path / "bad"), index=p.get("i1"))
    assert [f for f in os.listdir(tmp_path) if f.startswith("bad")] == []


@pytest.mark.parametrize("short_type", ["stlfr", "tellseq"])
def test_one_call_sort_equals_the_two_step_route(short_type, tmp_path):
    rng = random.Random(5)
    r1, r2, i1 = _random_units(rng, short_type, 700, lengths=(0, 36, 100))
    p = _files(tmp_path, r1=r1, r2=r2[:-1], **({"i1": i1} if i1 else {}))
    want = ref.preprocess(short_type, r1, r2, i1)
    prepared = ref.interleaved(want)
    units = _sort_ref.units_of(prepared)
    out = str(tmp_path / "one.fq")
    res = sortreads.sort_fastq(p["r1"], out, p["r2"], short_type=short_type, index=p.get("i1"))
    assert _read(out) == _sort_ref.sort_text(prepared)
    assert (res["short_type"], res["raw_pairs"], res["prepared_pairs"], res["pairs"]) == (short_type, 700, want["written"], want["written"])
    assert res["dropped_pairs"] == 700 - want["written"] and res["tagged_pairs"] == want["tagged"]
    assert res["barcodes"] == _sort_ref.barcodes(units) and res["untagged_pairs"] == sum(1 for u in units if u[0] is None)
    assert not res["already_sorted"] and res["bytes"] == len(prepared) and "prep" in res["device_ms"] and res["device_ms"]["prep"] > 0
    # the two-step route: preprocess_reads to files, then the sort as it was
    pre = str(tmp_path / "two")
    prepreads.preprocess_reads(short_type, p["r1"], p["r2"], pre, index=p.get("i1"))
    two = str(tmp_path / "two.sorted.fq")
    res2 = sortreads.sort_fastq(pre + "_1.fq", two, pre + "_2.fq")
    assert _read(two) == _read(out)
    assert "prep" not in res2["device_ms"] and "short_type" not in res2 and {k: res[k] for k in res2 if k not in ("seconds", "device_ms")} == {
        k: v for k, v in res2.items() if k not in ("seconds", "device_ms")}
    # --check on the raw input: unsorted, with the ordinal of the first descent among the prepared units
    chk = sortreads.check_fastq(p["r1"], p["r2"], short_type=short_type, index=p.get("i1"))
    assert (chk["sorted"], chk["first_descent"], chk["pairs"], chk["raw_pairs"]) == (False, _sort_ref.first_descent(units), want["written"], 700)
    # ... and on raw input whose prepared form is sorted: the raw units in the order of the sort
    order = _sort_ref.order(_sort_ref.units_of(ref.interleaved(want)))
    if short_type == "tellseq":                              # (the order is over KEPT units: sort those, drop the others)
        kept = [u for u, x in enumerate(ref.plan(short_type, r1, r2, i1)) if x[2]]
        order = [kept[i] for i in order]
    recs = [ref.records_of(d) for d in (r1, r2) + ((i1,) if i1 else ())]
    s = _files(tmp_path, **{"s%d" % f: b"".join(b"".join(x + b"\n" for x in rec[u]) for u in order) for f, rec in enumerate(recs)})
    chk = sortreads.check_fastq(s["s0"], s["s1"], short_type=short_type, index=s.get("s2"))
    assert (chk["sorted"], chk["first_descent"], chk["pairs"], chk["barcodes"]) == (True, None, len(order), res["barcodes"])
    # through the command line
    assert cli.main_sort_barcodes(["--check", "--short_type", short_type, "-1", s["s0"], "-2", s["s1"]] + (["-I", s["s2"]] if i1 else [])) == 0
    assert cli.main_sort_barcodes(["--short_type", short_type, "-1", p["r1"], "-2", p["r2"], "-o", str(tmp_path / "cli.fq")] + (["-I", p["i1"]] if i1 else [])) == 0
    assert _read(str(tmp_path / "cli.fq")) == _read(out)


def test_tellseq_input_in_which_every_unit_is_dropped(tmp_path, capsys):
    heads = [b"@t%d 1:N" % i for i in range(70)]
    p = _files(tmp_path, r1=b"".join(_rec(h) for h in heads), r2=b"".join(_rec(h, b"TT") for h in heads),
               i1=b"".join(_rec(b"@i", b"A" * (17 + 2 * (i % 2))) for i in range(70)))
    out = str(tmp_path / "none.fq")
    res = sortreads.sort_fastq(p["r1"], out, p["r2"], short_type="tellseq", index=p["i1"])
    assert _read(out) == b""
    assert (res["pairs"], res["barcodes"], res["untagged_pairs"], res["bytes"], res["raw_pairs"], res["dropped_pairs"], res["tagged_pairs"]) == (
        0, 0, 0, 0, 70, 70, 0)
    assert res["already_sorted"] and res["passes"] == 0
    chk = sortreads.check_fastq(p["r1"], p["r2"], short_type="tellseq", index=p["i1"])
    assert (chk["sorted"], chk["pairs"], chk["barcodes"], chk["dropped_pairs"]) == (True, 0, 0, 70)
    pre = str(tmp_path / "pre")
    res = prepreads.preprocess_reads("tellseq", p["r1"], p["r2"], pre, index=p["i1"])
    assert (res["pairs"], res["kept_pairs"], res["dropped_pairs"], res["bytes"]) == (70, 0, 70, 0)
    assert [_read(pre + s) for s in ("_1.fq", "_2.fq", ".wl")] == [b"", b"", b""]
    # files without a record
    e = _files(tmp_path, e1=b"", e2=b"", e3=b"")
    res = sortreads.sort_fastq(e["e1"], out, e["e2"], short_type="tellseq", index=e["e3"])
    assert _read(out) == b"" and (res["pairs"], res["raw_pairs"], res["bytes"]) == (0, 0, 0)
    res = prepreads.preprocess_reads("stlfr", e["e1"], e["e2"], pre)
    assert (res["pairs"], res["tagged_pairs"], res["bytes"]) == (0, 0, 0) and _read(pre + "_1.fq") == b""
    # refusals of the library calls themselves
    with pytest.raises(ValueError, match="index reads go with short_type tellseq only"):
        sortreads.sort_fastq(p["r1"], out, p["r2"], index=p["i1"])
    with pytest.raises(ValueError, match="not interleaved"):
        sortreads.sort_fastq(p["r1"], out, short_type="stlfr")
    with pytest.raises(ValueError, match="must be 10x, stlfr or tellseq"):
        sortreads.check_fastq(p["r1"], p["r2"], short_type="hybrid")
    short = _files(tmp_path, short=_rec(b"@i", b"A" * 18))["short"]
    with pytest.raises(ValueError, match=r"r1\.fq holds 70 records, .*short\.fq holds 1"):
        sortreads.sort_fastq(p["r1"], out, p["r2"], short_type="tellseq", index=short)


def test_features_of_raw_stlfr_reads_equal_those_of_the_prepared_sorted_file(tmp_path):
    """end to end: count_tnf on the raw interleaved stLFR file (header mode stLFR) and on the file the one-call sort makes of
    the raw R1 / R2 (header mode 10x) give the same CSV.  No barcode is partially zero -- such a pair is a barcode of its own
    to the stLFR header mode and untagged to the reference's preprocessing --, and the raw file stands in the order of the
    sort, so that the rows come in the same order."""
    cfg = synth.SynthConfig(n_pairs=3000, n_barcodes=38, n_genomes=2, genome_len=20_000, fragment=2_000, n_rate=0.1, unbarcoded=0.05, seed=5)
    stream = synth.generate(cfg)
    raw = str(tmp_path / "raw.fq")
    synth.write_fastq(stream, cfg, raw, style="stlfr")
    lines = ref.contents_of(_read(raw))
    pairs = [lines[i:i + 8] for i in range(0, len(lines), 8)]
    assert len(pairs) == 3000 and sum(1 for x in pairs if b"#0_0_0/" in x[0]) == 150

    def tag(x):
        b = x[0].split(b"#")[1].split(b"/")[0]
        return (b == b"0_0_0", b"BX:Z:" + b + b"-1")

    in_order = sorted(pairs, key=tag)                        # (stable: the input order within a barcode)
    ordered = str(tmp_path / "raw.ordered.fq")
    with open(ordered, "wb") as f:
        f.write(b"".join(b"".join(x + b"\n" for x in p) for p in in_order))
    # the sort's input: the same pairs dealt round-robin over the barcodes, the order within a barcode kept
    seen, dealt = {}, []
    for x in in_order:
        k = tag(x)
        seen[k] = seen.get(k, 0) + 1
        dealt.append((seen[k], len(dealt), x))
    dealt = [x for _, _, x in sorted(dealt, key=lambda t: t[:2])]
    p = _files(tmp_path, r1=b"".join(b"".join(y + b"\n" for y in x[:4]) for x in dealt), r2=b"".join(b"".join(y + b"\n" for y in x[4:]) for x in dealt))
    out = str(tmp_path / "interleaved.sorted.fastq")
    res = sortreads.sort_fastq(p["r1"], out, p["r2"], short_type="stlfr")
    assert (res["pairs"], res["barcodes"], res["untagged_pairs"], res["tagged_pairs"], res["already_sorted"]) == (3000, 38, 150, 2850, False)
    assert cli.main_count_tnf(["-i", ordered, "-o", str(tmp_path / "raw.csv.gz"), "-l", "1000"]) == 0
    assert cli.main_count_tnf(["-i", out, "-o", str(tmp_path / "sorted.csv.gz"), "-l", "1000"]) == 0
    a, b = (gzip.decompress(_read(str(tmp_path / n))) for n in ("raw.csv.gz", "sorted.csv.gz"))
    assert a == b and a.count(b"\n") >= 38
