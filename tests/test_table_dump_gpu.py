"""The table as jellyfish's text dump and back, on the GPU: ``KmerTable.write_dump`` (pg_table_dump_sizes / pg_table_dump_text),
``KmerTable.from_dump`` (pg_dump_parse), ``kmer_table dump``, ``count_kmer -g`` and ``Feature`` with PANGAEA_WRITE_DUMP=1.

Yardsticks: ``KmerTable.items()`` formatted on the host, ``cli.load_dump`` (the host statement of the loader semantics), the
oracle's own dump loader, and -- where oracle/_ref was built -- the reference's ``count_kmer`` binary reading a file written here.
Tables hold a few hundred entries: counts at every digit boundary, codes at the edges (all-A, self-complementary k-mers, the
largest canonical code), entries poked into the first and last slot of the table and of a unit, every table kind at the ends of
its k range."""
import argparse
import ctypes as C
import glob
import gzip
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import oracle
from pangaea_amd import _lib, cli, kmer
from pangaea_amd.kmer import KmerTable

from .conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAT = _lib.HASH_COUNT_SAT
UNIT = _lib.DUMP_UNIT_SLOTS
PACKED_COUNTS = [1, 9, 10, 99, 100, 999_999, 1_000_000, SAT]
WIDE_COUNTS = PACKED_COUNTS + [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2]


def _canon(code: int, k: int) -> int:
    return min(code, oracle.revcomp(code, k))


def _code_of(s: str) -> int:
    c = 0
    for ch in s:
        c = (c << 2) | "ACTG".index(ch)
    return c


def _chosen(k: int, wide: bool, n_random: int = 600, seed: int = 0):
    """(codes uint64 sorted, counts uint64) -- canonical codes: the edge cases first, then random ones; counts cycle the boundaries"""
    rng = np.random.RandomState(seed + k)
    h = k // 2
    special = [0, _code_of("G" * h + "C" * (k - h))]                      # all-A; the largest canonical code
    assert _canon(special[1], k) == special[1]
    special += [c for c in (UNIT - 1, UNIT, 2 * UNIT - 1) if c < 4 ** k and _canon(c, k) == c]     # dense: the edges of a unit
    if k % 2 == 0:
        special.append(_code_of(("ACGT" * 8)[:h] + "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(("ACGT" * 8)[:h]))))
        assert oracle.revcomp(special[-1], k) == special[-1]             # its own reverse complement
        if k % 4 == 0:
            special.append(_code_of("ACGT" * (k // 4)))
            assert oracle.revcomp(special[-1], k) == special[-1]
    rand = [_canon(int(x), k) for x in rng.randint(0, 1 << min(62, 2 * k), size=n_random, dtype=np.int64)] if k > 1 else [0, 1]
    codes = np.array(sorted(set(special + rand)), dtype=np.uint64)
    pool = WIDE_COUNTS if wide else PACKED_COUNTS
    counts = np.array([pool[i % len(pool)] for i in rng.permutation(len(codes))], dtype=np.uint64)
    return codes, counts


def _lines(codes, counts, k):
    return [f"{oracle.code_to_kmer(int(c), k)}\t{int(n)}\n".encode() for c, n in zip(codes, counts)]


def _poke(table: KmerTable, extra):
    """entries straight into chosen slots (the writer formats what a slot holds, wherever a count would have put it): the first
    and last slot of the table and of a unit, where they are free"""
    n = table.n_entries
    slots = [s for s in dict.fromkeys([0, UNIT - 1, UNIT, n - 1]) if 0 <= s < n]
    data = table.data
    for s, (code, cnt) in zip(slots, extra):
        if table.kind in ("wide", "miniw"):
            keys, cnts = table._wide_parts()
            if int(keys[s]) == 0:
                keys[s] = code + 1
                cnts[s] = cnt
        elif int(data[s]) == 0:
            key = int(kmer.key42(np.array([code], np.uint64))[0]) if table.kind == "hash" else code
            slot = (key << _lib.HASH_COUNT_BITS) | cnt
            data[s] = slot - (1 << 64) if slot >= 1 << 63 else slot      # (the int64 with those bits)
    table._empty = False


def _build(kind: str, k: int, log2_slots):
    wide = kind in ("wide", "miniw")
    codes, counts = _chosen(k, wide)
    if kind == "hash":                                                   # a chosen geometry: 2^12 unbucketed, 2^15 bucketed
        t = KmerTable.with_slots(k, DEV, log2_slots)
        assert bool(t.log2_bucket) == (log2_slots >= 14)
        keys = torch.from_numpy(kmer.key42(codes).view(np.int64))
        t.merge((keys << _lib.HASH_COUNT_BITS) | torch.from_numpy(counts.view(np.int64)))
    elif kind == "miniw" and log2_slots:                                 # ... more than a few units of keys + counts planes
        t = KmerTable.mini_with_slots(k, DEV, log2_slots)
        c = torch.from_numpy(codes.view(np.int64)).to(DEV)
        n = torch.from_numpy(counts.view(np.int64)).to(DEV, torch.int32)
        _lib.check(_lib.load().pg_kmer_merge_wide(c.data_ptr(), n.data_ptr(), c.numel(), t.desc(), t.status.data_ptr(), None))
        torch.cuda.synchronize()
        t._empty = False
        t.check_status()
    else:
        t = KmerTable.from_items(k, codes, counts, DEV, kind=kind)
    assert t.kind == kind
    if kind != "dense":
        # four more canonical codes that the set does not hold
        have, extra, x = set(codes.tolist()), [], 12345
        while len(extra) < 4:
            x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
            c = _canon(x >> (64 - 2 * k), k)
            if c not in have:
                have.add(c)
                extra.append((c, [7, 10, SAT, 123456][len(extra)]))
        _poke(t, extra)
    return t


KINDS = ([("dense", k, None) for k in (1, 4, 8)] + [("hash", k, s) for k in (9, 15, 21) for s in (12, 15)]
         + [("mini", k, None) for k in (13, 16, 21)] + [("wide", k, None) for k in (22, 31)] + [("miniw", k, None) for k in (22, 27, 31)])


def _write(table, path, monkeypatch, piece=None, lower=1):
    if piece is None:
        monkeypatch.delenv("PG_DUMP_PIECE_BYTES", raising=False)
    else:
        monkeypatch.setenv("PG_DUMP_PIECE_BYTES", str(piece))
    got = table.write_dump(str(path), lower=lower)
    assert not os.path.exists(str(path) + ".tmp")
    return got, open(path, "rb").read()


@pytest.mark.parametrize("kind,k,log2_slots", KINDS)
def test_writer_every_kind(kind, k, log2_slots, tmp_path, monkeypatch):
    t = _build(kind, k, log2_slots)
    codes, counts = t.items()
    want = _lines(codes, counts, k)
    assert len(want) >= (2 if k == 1 else 100)
    (lines, nbytes), text = _write(t, tmp_path / "one.dump", monkeypatch)
    assert text.endswith(b"\n") and lines == len(want) and nbytes == len(text) == sum(map(len, want))
    got = text.splitlines(keepends=True)
    assert len(got) == len(want) and set(got) == set(want)
    if kind == "dense":
        assert got == want                                               # slot order is code order there
    # the oracle's loader reads the file to the same items
    ocodes, ocounts = oracle.Table.from_dump(str(tmp_path / "one.dump"), k).items()
    assert np.array_equal(ocodes, codes) and np.array_equal(ocounts, counts)
    # small pieces (they start mid-table, at unaligned offsets): the same bytes
    (lines2, nbytes2), text2 = _write(t, tmp_path / "pieces.dump", monkeypatch, piece=4096)
    assert (lines2, nbytes2) == (lines, nbytes) and text2 == text
    # -L: exactly the entries below are left out, the others keep their order
    for lower in (2, 10):
        (ln, nb), low = _write(t, tmp_path / f"low{lower}.dump", monkeypatch, piece=4096 if lower == 2 else None, lower=lower)
        keep = [line for line in got if int(line.split(b"\t")[1]) >= lower]
        assert low == b"".join(keep) and ln == len(keep) and nb == len(low) and len(keep) < len(got) and (keep or k == 1)
    # the table is untouched
    c2, n2 = t.items()
    assert np.array_equal(c2, codes) and np.array_equal(n2, counts)


@pytest.mark.parametrize("kind,k", [("dense", 4), ("hash", 15), ("mini", 21), ("wide", 31), ("miniw", 22)])
def test_empty_and_reset_tables_write_nothing(kind, k, tmp_path, monkeypatch):
    t = KmerTable.alloc(k, DEV, kind, distinct_hint=1 << 14)
    (lines, nbytes), text = _write(t, tmp_path / "empty.dump", monkeypatch)
    assert (lines, nbytes, text) == (0, 0, b"")
    codes, counts = _chosen(k, False, n_random=200)
    t = KmerTable.from_items(k, codes, counts, DEV, kind=kind)
    assert _write(t, tmp_path / "full.dump", monkeypatch)[0][0] == len(codes)
    t.reset()
    (lines, nbytes), text = _write(t, tmp_path / "reset.dump", monkeypatch)
    assert (lines, nbytes, text) == (0, 0, b"")


@pytest.mark.parametrize("kind,k,log2_slots", [("hash", 21, 15), ("miniw", 27, 14), ("dense", 8, None)])
def test_text_kernel_stores_nothing_outside_its_range(kind, k, log2_slots, tmp_path, monkeypatch):
    """an inner unit range into a buffer with 4 KiB guards and a pre-filled body, the text pointer not even 2-byte aligned: the
    range's bytes are the file's, every other byte keeps its fill"""
    t = _build(kind, k, log2_slots)
    _, whole = _write(t, tmp_path / "whole.dump", monkeypatch)
    L = _lib.load()
    n_units = L.pg_table_dump_units(t.desc())
    assert n_units >= 16
    sizes = torch.empty(n_units, dtype=torch.int64, device=DEV)
    _lib.check(L.pg_table_dump_sizes(t.desc(), 1, sizes.data_ptr(), None, None))
    offsets = torch.cat([sizes.new_zeros(1), torch.cumsum(sizes, 0)])
    off = offsets.cpu().numpy()
    assert off[-1] == len(whole)
    guard, slack, skew = 4096, 300, 7
    for a, b in ((5, 11), (0, 3), (n_units - 2, n_units), (7, 8)):
        nb = int(off[b] - off[a])
        assert nb > 0
        buf = torch.full((guard + skew + nb + slack + guard,), 0x5A, dtype=torch.uint8, device=DEV)
        buf[:guard] = 0xA5
        buf[-guard:] = 0xA5
        _lib.check(L.pg_table_dump_text(t.desc(), 1, a, b, offsets.data_ptr(), int(off[a]), nb, buf.data_ptr() + guard + skew, nb + slack, None))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:guard] == 0xA5).all() and (got[-guard:] == 0xA5).all()
        assert (got[guard:guard + skew] == 0x5A).all() and (got[guard + skew + nb:-guard] == 0x5A).all()
        assert got[guard + skew:guard + skew + nb].tobytes() == whole[int(off[a]):int(off[b])]
    # offsets that claim more than the host was told: the stores stop at range_bytes
    buf = torch.full((guard + 64 + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    _lib.check(L.pg_table_dump_text(t.desc(), 1, 5, 11, offsets.data_ptr(), int(off[5]), 64, buf.data_ptr() + guard, 64, None))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:guard] == 0x5A).all() and (got[guard + 64:] == 0x5A).all()


# ------------------------------------------------------------------------------------------------ the parser

def _k_of(path):
    return int(re.search(r"\.k(\d+)\.", os.path.basename(path)).group(1))


GOLDEN_DUMPS = sorted(glob.glob(os.path.join(GOLDEN, "*.dump")))
_REFS = {}


def _refs(path):
    """(items of from_items(load_dump), items of the oracle's loader clamped as the kind stores them): computed once per file"""
    if path not in _REFS:
        k = _k_of(path)
        t = KmerTable.from_items(k, *cli.load_dump(path, k), DEV)
        ocodes, ocounts = oracle.Table.from_dump(path, k).items()
        if t.kind in ("hash", "mini"):
            ocounts = np.minimum(ocounts, np.uint64(SAT))
        _REFS[path] = (t.kind, t.log2_slots, t.items(), (ocodes, ocounts))
    return _REFS[path]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("piece", [None, 4096, 4099])
@pytest.mark.parametrize("path", GOLDEN_DUMPS, ids=os.path.basename)
def test_parser_against_both_yardsticks(path, piece, monkeypatch):
    if piece is None:
        monkeypatch.delenv("PG_DUMP_PIECE_BYTES", raising=False)
    else:
        monkeypatch.setenv("PG_DUMP_PIECE_BYTES", str(piece))
    kind, log2_slots, want, owant = _refs(path)
    t = KmerTable.from_dump(path, _k_of(path), DEV)
    assert (t.kind, t.log2_slots) == (kind, log2_slots)
    got = t.items()
    assert len(got[0]) > 0 and _same(got, want) and _same(got, owant)


def _load(tmp_path, monkeypatch, text: bytes, k: int, piece=None, kind=None):
    p = tmp_path / f"t{len(os.listdir(tmp_path))}.dump"
    p.write_bytes(text)
    if piece is None:
        monkeypatch.delenv("PG_DUMP_PIECE_BYTES", raising=False)
    else:
        monkeypatch.setenv("PG_DUMP_PIECE_BYTES", str(piece))
    return str(p), KmerTable.from_dump(str(p), k, DEV, kind)


def _items_dict(t):
    codes, counts = t.items()
    return {int(c): int(n) for c, n in zip(codes, counts)}


def _filler(k, n, seed=3):
    """n regular lines of distinct canonical k-mers (counts 1..), as (bytes, {code: count})"""
    codes = _chosen(k, False, n_random=2 * n, seed=seed)[0][:n]
    return b"".join(_lines(codes, range(1, len(codes) + 1), k)), {int(c): i + 1 for i, c in enumerate(codes)}


@pytest.mark.parametrize("piece", [None, 256, 263])
def test_parser_edge_cases(piece, tmp_path, monkeypatch):
    k = 15
    body, want = _filler(k, 300)
    # no trailing newline; CRLF; blank lines (also "\r\n" ones, also at the very start and end)
    for text in (body[:-1], body.replace(b"\n", b"\r\n"), b"\n\r\n" + body.replace(b"\n", b"\n\n", 40) + b"\n\n", body.replace(b"\n", b"\r\n")[:-2]):
        path, t = _load(tmp_path, monkeypatch, text, k, piece)
        assert _items_dict(t) == want
        assert _same(t.items(), KmerTable.from_items(k, *cli.load_dump(path, k), DEV).items())
    # a k-mer given three times, far apart and on both strands: the last line wins
    lines = body.splitlines(keepends=True)
    code = next(iter(want))
    fw = oracle.code_to_kmer(code, k)
    rc = oracle.code_to_kmer(oracle.revcomp(code, k), k)
    assert fw != rc
    dup = [f"{rc}\t777\n".encode()] + lines[:200] + [f"{fw}\t888\n".encode()] + lines[200:] + [f"{rc}\t999\n".encode()]
    _, t = _load(tmp_path, monkeypatch, b"".join(dup), k, piece)
    assert _items_dict(t) == {**want, code: 999}
    _, t = _load(tmp_path, monkeypatch, b"".join(dup[:-1]), k, piece)
    assert _items_dict(t) == {**want, code: 888}
    # N and lower case: dropped, the neighbours stay
    odd = lines[:50] + [b"ACGTNACGTACGTAC\t5\n", b"acgtacgtacgtacg\t6\n", b"ACGTACGTACGTACg\t7\r\n"] + lines[50:]
    _, t = _load(tmp_path, monkeypatch, b"".join(odd), k, piece)
    assert _items_dict(t) == want
    # 18 digits (a wide table keeps the low 32 bits, as from_items of the same pair does)
    big = 10 ** 18 - 1
    _, t = _load(tmp_path, monkeypatch, body + f"{fw}\t{big}\n".encode(), k, piece)
    assert _items_dict(t) == {**want, code: SAT}
    kw = 31
    wcode = _chosen(kw, True, 10)[0][5]
    text = f"{oracle.code_to_kmer(int(wcode), kw)}\t{big}\n".encode()
    _, t = _load(tmp_path, monkeypatch, text, kw, piece)
    assert _items_dict(t) == {int(wcode): big & 0xFFFFFFFF} == _items_dict(KmerTable.from_items(kw, [wcode], [big], DEV))
    # an empty file, one line with and without its newline
    _, t = _load(tmp_path, monkeypatch, b"", k, piece)
    assert _items_dict(t) == {} and t.kind == "hash" and t.log2_slots == KmerTable.from_items(k, [], [], DEV).log2_slots
    for text in (lines[0], lines[0][:-1], lines[0][:-1] + b"\r\n", lines[0][:-1] + b"\r"):
        _, t = _load(tmp_path, monkeypatch, text, k, piece)
        assert lines[0].startswith(fw.encode()) and _items_dict(t) == {code: want[code]}


BAD = [
    ("ACGTACGTACGTAC\t5", "length is not 15"),                            # k - 1 characters
    ("ACGTACGTACGTACGT\t5", "length is not 15"),                          # k + 1
    ("ACGTACGTACGTACG 5", "no TAB"),
    ("ACGTACGTACGTACG", "no TAB"),
    ("ACGTACGTACGTACG\t", "count"),
    ("ACGTACGTACGTACG\t-3", "count"),
    ("ACGTACGTACGTACG\t12x", "count"),
    ("ACGTACGTACGTACG\t12\t7", "count"),
    ("ACGTACGTACGTACG\t 12", "count"),
    ("ACGTACGTACGTACG\t1234567890123456789", "count"),                    # 19 digits
    ("NCGTACGTACGTACG\t", "count"),                                       # a dropped k-mer's count is still read
    ("ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\t5", "length is not 15"),
]


@pytest.mark.parametrize("bad,text", BAD, ids=[repr(b[0])[:28] for b in BAD])
def test_parser_refusals_name_the_line(bad, text, tmp_path, monkeypatch):
    k = 15
    body, _ = _filler(k, 120)
    lines = body.splitlines(keepends=True)
    for piece in (None, 256):
        for at, ending in ((0, b"\n"), (77, b"\r\n"), (len(lines), b"\n"), (len(lines), b"")):
            blanks = 2 if at else 0                                       # blank lines count as lines
            doc = b"".join(lines[:at][:40]) + b"\n" * blanks + b"".join(lines[:at][40:]) + bad.encode() + ending + b"".join(lines[at:])
            p = tmp_path / "bad.dump"
            p.write_bytes(doc)
            if piece is None:
                monkeypatch.delenv("PG_DUMP_PIECE_BYTES", raising=False)
            else:
                monkeypatch.setenv("PG_DUMP_PIECE_BYTES", str(piece))
            with pytest.raises(ValueError) as e:
                KmerTable.from_dump(str(p), k, DEV)
            msg = str(e.value)
            assert text in msg and re.search(rf"\bline {at + blanks + 1}\b", msg) and str(p) in msg, msg
    # two bad lines: the first is reported
    p.write_bytes(b"".join(lines[:30]) + b"ACGT\t1\n" + b"".join(lines[30:60]) + b"ACGTACGTACGTACG\tx\n")
    with pytest.raises(ValueError, match=r"length is not 15 \(line 31\)"):
        KmerTable.from_dump(str(p), k, DEV)


# ------------------------------------------------------------------------------------------------ round trips and tools

@pytest.mark.parametrize("fq,k", [("tenx_mixed.fq", 15), ("tenx_mixed.fq", 21), ("tenx_hashbx.fq", 31)])
def test_round_trip_of_counted_tables(fq, k, tmp_path, monkeypatch):
    from pangaea_amd.reads import ReadStream
    s = ReadStream.from_fastq(os.path.join(GOLDEN, fq), None, device=DEV).to(DEV)
    t = kmer.count_kmers(s, k)
    (lines, nbytes), text = _write(t, tmp_path / "t.dump", monkeypatch, piece=1 << 14)
    codes, counts = t.items()
    assert lines == len(codes) > 100
    monkeypatch.setenv("PG_DUMP_PIECE_BYTES", "5003")
    back = KmerTable.from_dump(str(tmp_path / "t.dump"), k, DEV)
    assert _same(back.items(), (codes, counts))
    q = torch.from_numpy(codes.view(np.int64)).to(DEV)
    assert torch.equal(back.query(q), t.query(q)) and np.array_equal(back.query(q).cpu().numpy().astype(np.uint64), counts)
    assert np.array_equal(back.spectrum(100), t.spectrum(100))
    # and what was counted is what the oracle counts
    ocodes, ocounts = oracle.Table.from_dump(str(tmp_path / "t.dump"), k).items()
    want = oracle.Table(k).count(oracle.Reads(os.path.join(GOLDEN, fq)).all_seq(), lowercase_is_base=False).items()
    assert _same((ocodes, ocounts), want)


def test_kmer_table_dump_feeds_histo_and_count_kmer(tmp_path, capsys):
    fq = os.path.join(GOLDEN, "tenx_mixed.fq")
    out = str(tmp_path / "k15.dump")
    assert cli.main_kmer_table(["dump", "-i", fq, "-k", "15", "-o", out]) == 0
    assert cli.main_kmer_table(["histo", "-g", out, "-k", "15", "-o", str(tmp_path / "a.histo")]) == 0
    assert cli.main_kmer_table(["histo", "-i", fq, "-k", "15", "-o", str(tmp_path / "b.histo")]) == 0
    a, b = open(tmp_path / "a.histo").read(), open(tmp_path / "b.histo").read()
    assert a == b and a.startswith("1 ")
    # -L through the tool, on a table with a spread of counts (a dump of a dump: dense tables write in code order); the file
    # holds 512 lines with counts up to 22, 188 of them at 10 or above
    k5 = os.path.join(GOLDEN, "tenx_mixed.k5.dump")
    for lower in (1, 10):
        assert cli.main_kmer_table(["dump", "-g", k5, "-k", "5", "-L", str(lower), "-o", str(tmp_path / "l.dump")]) == 0
        low = open(tmp_path / "l.dump", "rb").read().splitlines()
        want = sorted(x for x in open(k5, "rb").read().splitlines() if int(x.split(b"\t")[1]) >= lower)
        assert 0 < len(low) == len(want) and sorted(low) == want and (lower == 1 or len(low) < 512)
    # count_kmer -g <the file>: the reference's abundance bytes
    gz = str(tmp_path / "abd.gz")
    assert cli.main_count_kmer(["-i", fq, "-g", out, "-k", "15", "-w", "1", "-v", "6", "-l", "100", "-o", gz]) == 0
    capsys.readouterr()
    with gzip.open(gz, "rb") as f, open(os.path.join(GOLDEN, "tenx_mixed.abd.k15.w1.v6.l100.csv"), "rb") as g:
        assert f.read() == g.read()
    # a malformed dump: exit status 1, the line on stderr
    bad = tmp_path / "bad.dump"
    bad.write_bytes(open(out, "rb").read() + b"ACGT\t1\n")
    n = len(open(out, "rb").read().splitlines())
    assert cli.main_count_kmer(["-i", fq, "-g", str(bad), "-k", "15", "-w", "1", "-v", "6", "-l", "100", "-o", gz]) == 1
    assert f"(line {n + 1})" in capsys.readouterr().err


def _args(tmp_path, **kw):
    d = dict(reads1="", reads2="", interleaved_reads="", output=str(tmp_path / "out"), min_length=100, kmer=15,
             tnf_kmer=4, window_size=1, vector_size=6, threads=4)
    d.update(kw)
    os.makedirs(d["output"], exist_ok=True)
    return argparse.Namespace(**d)


def test_feature_writes_the_dump_only_when_asked(tmp_path, monkeypatch):
    from pangaea_amd.feature import Feature
    fq = os.path.join(GOLDEN, "tenx_mixed.fq")
    monkeypatch.delenv("PANGAEA_WRITE_DUMP", raising=False)
    args = _args(tmp_path / "off", interleaved_reads=fq)
    names0, abd0, tnf0 = Feature(args, ROOT).extract_features()
    assert not glob.glob(os.path.join(args.output, "1.features", "*.dump*"))
    monkeypatch.setenv("PANGAEA_WRITE_DUMP", "1")
    args = _args(tmp_path / "on", interleaved_reads=fq)
    names, abd, tnf = Feature(args, ROOT).extract_features()
    assert (names == names0).all() and np.array_equal(abd, abd0) and np.array_equal(tnf, tnf0)
    dump = os.path.join(args.output, "1.features", "abundance.k15.dump")
    assert os.path.isfile(dump) and not os.path.exists(dump + ".tmp")
    assert sorted(os.listdir(os.path.join(tmp_path / "off", "out", "1.features")) + ["abundance.k15.dump"]) == sorted(os.listdir(os.path.dirname(dump)))
    want = oracle.Table(15).count(oracle.Reads(fq).all_seq(), lowercase_is_base=True).items()
    assert _same(oracle.Table.from_dump(dump, 15).items(), want)


@pytest.mark.skipif(oracle.ref_tool("count_kmer") is None, reason="oracle/_ref not built (needs the reference's sources at build time)")
def test_reference_count_kmer_reads_a_dump_written_here(tmp_path, monkeypatch):
    from pangaea_amd.reads import ReadStream
    fq = os.path.join(GOLDEN, "tenx_mixed.fq")
    s = ReadStream.from_fastq(fq, None, device=DEV).to(DEV)
    dump = tmp_path / "k15.dump"
    _write(kmer.count_kmers(s, 15), dump, monkeypatch, piece=1 << 14)
    gz = str(tmp_path / "ref.gz")
    subprocess.run([oracle.ref_tool("count_kmer"), "-i", fq, "-g", str(dump), "-k", "15", "-w", "1", "-v", "6", "-l", "100", "-t", "2", "-o", gz],
                   check=True, stdout=subprocess.DEVNULL)
    with gzip.open(gz, "rb") as f, open(os.path.join(GOLDEN, "tenx_mixed.abd.k15.w1.v6.l100.csv"), "rb") as g:
        assert f.read() == g.read()
