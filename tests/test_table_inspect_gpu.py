"""Asking a finished table: ``KmerTable.query`` / ``KmerTable.spectrum`` (pg_table_query, pg_table_spectrum) and the ``kmer_table``
tool -- what `jellyfish query` / `jellyfish histo` give from the dump the reference keeps (src/feature.py:87,103).

Integer results, compared exactly: every multiplicity and every spectrum against ``oracle.Table(k).count(text).items()``, for all
five table kinds at the edges of their k ranges, whatever the placement (index, key42, mix64, minimizer buckets) and the probe
order of the kind are.  One stream, one oracle table and one device table per case, shared by the tests below."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from pangaea_amd import _lib, cli, kmer, synth
from pangaea_amd.reads import ReadStream

from .conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAT = _lib.HASH_COUNT_SAT
HIGHS = (1, 2, 255, 10000, 16382)

# (kind, k, log2_slots, log2_bucket): every kind, the edges of its k range, tables with one bucket and with thousands
CASES = [("dense", 4, 0, 0), ("dense", 8, 0, 0),
         ("hash", 11, 12, 0),                      # unbucketed: probing runs through the whole table
         ("hash", 21, 20, 10),                     # bucketed: probing wraps inside a bucket
         ("wide", 22, 20, 0), ("wide", 31, 20, 0),
         ("mini", 13, 18, 12), ("mini", 15, 20, 10), ("mini", 21, 22, 10), ("mini", 21, 14, 14),
         ("miniw", 22, 20, 13), ("miniw", 31, 20, 13)]
_IDS = [f"{c[0]}-k{c[1]}-s{c[2]}-b{c[3]}" for c in CASES]


def _rc(codes, k):
    """reverse complement of codes (complement = ^ 2 per character, A0 C1 T2 G3)"""
    c = np.asarray(codes, dtype=np.uint64).copy()
    out = np.zeros_like(c)
    for _ in range(k):
        out = (out << np.uint64(2)) | ((c & np.uint64(3)) ^ np.uint64(2))
        c >>= np.uint64(2)
    return out


def _canon(codes, k):
    return np.minimum(codes, _rc(codes, k))


def _strings(codes, k):
    sh = (2 * np.arange(k - 1, -1, -1)).astype(np.uint64)
    digits = ((np.asarray(codes, dtype=np.uint64)[:, None] >> sh[None, :]) & np.uint64(3)).astype(np.int64)
    chars = np.ascontiguousarray(np.frombuffer(b"ACTG", dtype=np.uint8)[digits])
    return chars.view(f"S{k}").ravel().astype(str).tolist()


def _stream(kind, k, log2_slots):
    if kind == "hash" and log2_slots == 12:
        # few enough distinct 11-mers for 2^12 slots: one small genome, no substitutions (the table ends up more than half full)
        cfg = synth.SynthConfig(n_pairs=800, n_barcodes=37, n_genomes=1, genome_len=2_600, fragment=2_000, sub_rate=0.0, n_rate=0.2, seed=500 + k)
    elif log2_slots == 14:
        cfg = synth.SynthConfig(n_pairs=40, n_barcodes=2, n_genomes=3, genome_len=30_000, fragment=8_000, sub_rate=0.01, n_rate=0.2, seed=500 + k)
    else:
        cfg = synth.SynthConfig(n_pairs=1000, n_barcodes=37, n_genomes=3, genome_len=30_000, fragment=8_000, sub_rate=0.01, n_rate=0.2, seed=500 + k)
    return synth.generate(cfg, device=DEV)


@functools.lru_cache(maxsize=None)
def _built(case):
    """(table, oracle codes, the counts the table must hold) of a case"""
    kind, k, log2_slots, log2_bucket = case
    s = _stream(kind, k, log2_slots)
    if kind == "dense":
        t = kmer.KmerTable.alloc(k, DEV, "dense")
    elif kind == "hash":
        t = kmer.KmerTable.with_slots(k, DEV, log2_slots, log2_bucket)
    elif kind == "wide":
        t = kmer.KmerTable.wide_with_slots(k, DEV, log2_slots)
    else:
        t = kmer.KmerTable.mini_with_slots(k, DEV, log2_slots, log2_bucket)
    t.count(s)
    assert t.kind == kind
    ocodes, ocounts = oracle.Table(k, threads=4).count(s.decode()).items()
    return t, ocodes, ocounts.astype(np.int64)


def _query_set(k, ocodes, ocounts, seed):
    """(codes uint64, expected int64): every k-mer of the table, its other strand, as many random absent ones, duplicates"""
    rng = np.random.RandomState(seed)
    rnd = _canon(rng.randint(0, 1 << 62, size=len(ocodes), dtype=np.int64).astype(np.uint64) & np.uint64((1 << (2 * k)) - 1), k)
    rnd = rnd[~np.isin(rnd, ocodes)]                     # (dense k = 4: every 4-mer may be present -- then none is left)
    flip = rng.rand(len(rnd)) < 0.5
    rnd = np.where(flip, _rc(rnd, k), rnd)               # absent k-mers of either strand
    dup = rng.randint(0, len(ocodes), size=257)
    codes = np.concatenate([ocodes, _rc(ocodes, k), rnd, ocodes[dup], _rc(ocodes[dup], k), rnd[:50], rnd[:50]])
    want = np.concatenate([ocounts, ocounts, np.zeros(len(rnd), np.int64), ocounts[dup], ocounts[dup], np.zeros(2 * len(rnd[:50]), np.int64)])
    order = rng.permutation(len(codes))
    return codes[order], want[order]


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_query_every_kind_and_the_edges_of_k(case):
    kind, k = case[0], case[1]
    t, ocodes, ocounts = _built(case)
    assert len(ocodes) > 100
    codes, want = _query_set(k, ocodes, ocounts, seed=k)
    bad = np.uint64(1 << (2 * k)) | codes[0]             # a bit at 2k: not a k-mer
    codes = np.concatenate([codes[:7], [bad], codes[7:]])
    want = np.concatenate([want[:7], [-1], want[7:]])
    dev = torch.from_numpy(codes.view(np.int64)).to(DEV)
    got = t.query(dev)
    assert got.dtype == torch.int64 and got.device == dev.device and got.shape == dev.shape
    assert np.array_equal(got.cpu().numpy(), want)
    # batches around the wavefront size, from slices of the device tensor (no host round trip), and nothing at all
    at = 0
    for n in (0, 1, 63, 64, 65, 1, 0, 64):
        part = t.query(dev[at:at + n])
        assert part.shape == (n,) and np.array_equal(part.cpu().numpy(), want[at:at + n])
        at += n
    assert np.array_equal(t.query(dev.view(torch.uint64)).cpu().numpy(), want)
    assert np.array_equal(t.query(codes).cpu().numpy(), want)                              # numpy, uint64
    # a code with the top bit set (negative as int64) is as invalid as any
    assert t.query(np.array([1 << 63, (1 << 64) - 1], dtype=np.uint64)).tolist() == [-1, -1]
    # the same questions as strings
    ok = want >= 0
    assert np.array_equal(t.query(_strings(codes[ok], k)).cpu().numpy(), want[ok])
    assert t.query([]).shape == (0,)
    with pytest.raises(ValueError):
        t.query(["A" * (k + 1)])
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        t.query(dev.cpu())
    # the table was only read
    assert all(np.array_equal(x, y) for x, y in zip(t.items(), (ocodes, np.minimum(ocounts, SAT).astype(np.uint64) if kind in ("hash", "mini") else ocounts.astype(np.uint64))))


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_spectrum_every_kind(case):
    t, ocodes, ocounts = _built(case)
    for high in HIGHS:
        hist = t.spectrum(high)
        assert hist.dtype == np.int64 and hist.shape == (high + 2,)
        assert np.array_equal(hist, np.bincount(np.minimum(ocounts, high + 1), minlength=high + 2))
        assert hist[0] == 0 and hist.sum() == len(ocodes)
    assert np.array_equal(t.spectrum(), t.spectrum(10000))
    for high in (0, 16383, -1):
        with pytest.raises(ValueError):
            t.spectrum(high)


def test_spectrum_of_empty_tables_and_of_a_table_counted_over_garbage():
    for k in (1, 2, 8):
        assert not kmer.KmerTable.alloc(k, DEV, "dense").spectrum(300).any()
    for t in (kmer.KmerTable.with_slots(21, DEV, 12, 0), kmer.KmerTable.wide_with_slots(25, DEV, 10), kmer.KmerTable.mini_with_slots(21, DEV, 4, 4),
              kmer.KmerTable.mini_with_slots(25, DEV, 4, 4)):
        assert not t.spectrum(300).any() and t.query(np.arange(5, dtype=np.uint64)).tolist() == [0] * 5
    # a mini table's memory is never cleared before the count: every slot is overwritten
    for k, log2_slots, log2_bucket in ((21, 22, 10), (22, 20, 13)):
        cfg = synth.SynthConfig(n_pairs=1000, n_barcodes=37, n_genomes=3, genome_len=30_000, fragment=8_000, sub_rate=0.01, n_rate=0.2, seed=500 + k)
        s = synth.generate(cfg, device=DEV)
        t = kmer.KmerTable.mini_with_slots(k, DEV, log2_slots, log2_bucket)
        t.data.fill_(0x7FFF_FFFF_FFFF)
        t.count(s)
        _, ocodes, ocounts = _built(("mini" if k <= 21 else "miniw", k, log2_slots, log2_bucket))      # the same stream
        for high in (2, 10000):
            assert np.array_equal(t.spectrum(high), np.bincount(np.minimum(ocounts, high + 1), minlength=high + 2))
        assert np.array_equal(t.query(ocodes).cpu().numpy(), ocounts)
        # ... and a reset() bucketed table is logically empty whatever its memory holds
        t.reset()
        assert not t.spectrum(100).any() and not t.query(ocodes[:1000]).any()


def _mini_slot_in_bucket(codes, log2_bucket):
    """the home slot of a code inside its bucket (pg_device.hpp: mini_slot_hash) -- restated here to read the layout from t.data"""
    c = np.asarray(codes, dtype=np.uint64)
    m24, m32 = np.uint64(0xFFFFFF), np.uint64(0xFFFFFFFF)
    x = (((c & m24) * np.uint64(0x9E3779)) ^ (((c >> np.uint64(21)) & m24) * np.uint64(0xC2B2AF)) ^ (((c >> np.uint64(45)) & m24) * np.uint64(0x85EBCB))) & m32
    x ^= x >> np.uint64(15)
    return x & np.uint64((1 << log2_bucket) - 1)


def test_probe_chains_that_wrap_inside_a_bucket(monkeypatch):
    """buckets of 2^4 slots: an entry whose home is near the end of its bucket sits at the bucket's beginning"""
    k = 21
    monkeypatch.setenv("PG_MINI_LOG2_BUCKET", "4")
    rng = np.random.RandomState(5)
    codes = np.unique(_canon(rng.randint(0, 1 << 42, size=700, dtype=np.int64).astype(np.uint64), k))
    counts = rng.randint(1, 1000, size=len(codes)).astype(np.uint64)
    t = kmer.KmerTable.from_items(k, codes, counts, DEV, "mini")               # 2^11 slots: 128 buckets of 16
    assert t.kind == "mini" and t.log2_bucket == 4 and t.log2_slots == 11
    slots = t.data.cpu().numpy().view(np.uint64)
    at = np.nonzero(slots)[0]
    assert len(at) == len(codes)
    home = _mini_slot_in_bucket(slots[at] >> np.uint64(22), 4).astype(np.int64)
    assert ((at & 15) < home).any(), "no probe chain wrapped: choose other items"
    assert ((at & 15) != home).sum() > 20
    assert np.array_equal(t.query(codes).cpu().numpy(), counts.astype(np.int64))
    assert np.array_equal(t.query(_rc(codes, k)).cpu().numpy(), counts.astype(np.int64))
    near = _canon(np.concatenate([codes ^ np.uint64(1), codes ^ np.uint64(1 << 20), codes ^ np.uint64(3 << 40)]), k)
    near = near[~np.isin(near, codes)]
    assert len(near) > 1500 and not t.query(near).any()
    assert np.array_equal(t.spectrum(1000), np.bincount(counts.astype(np.int64), minlength=1002))


@pytest.mark.parametrize("k,kind", [(21, "mini"), (21, "hash"), (22, "wide"), (25, "miniw")])
def test_saturating_counts(k, kind):
    """3.1 M copies of one k-mer: the packed count stops at HASH_COUNT_SAT, the wide layouts count on; ``query`` returns what the
    table holds and the spectrum puts it above ``high``"""
    s = ReadStream.from_runs([("a", b"A" * 1_600_000 + b"N" + b"T" * 1_500_040 + b"N"),
                              ("b", b"AC" * 40_000 + b"N" + b"ACG" * 30_000 + b"N" + b"AACCGGTT" * 9_000 + b"N")], device=DEV)
    t = kmer.count_kmers(s, k, kind=kind)
    assert t.kind == kind
    codes, counts = t.items()
    ocodes, ocounts = oracle.Table(k, threads=4).count(s.decode()).items()
    assert np.array_equal(codes, ocodes) and ocounts.max() > 3_000_000
    if kind in ("mini", "hash"):
        assert counts.max() >= SAT and np.array_equal(np.minimum(counts, SAT), np.minimum(ocounts, SAT))
    else:
        assert np.array_equal(counts, ocounts) and counts.max() > (1 << 21)
    assert np.array_equal(t.query(codes).cpu().numpy(), counts.astype(np.int64))
    assert np.array_equal(t.query(_rc(codes, k)).cpu().numpy(), counts.astype(np.int64))
    for high in (1, 255, 16382):
        hist = t.spectrum(high)
        assert np.array_equal(hist, np.bincount(np.minimum(ocounts, high + 1).astype(np.int64), minlength=high + 2))
        assert hist[high + 1] >= 1 and hist.sum() == len(ocodes)


def test_mid_size_table_of_the_default_geometry():
    cfg = synth.SynthConfig(n_pairs=60_000, n_barcodes=700, n_genomes=5, genome_len=60_000, fragment=20_000, sub_rate=0.01, n_rate=0.1, seed=77)
    s = synth.generate(cfg, device=DEV)
    t = kmer.count_kmers(s, 21)
    codes, counts = t.items()
    assert len(codes) > 1_000_000
    rng = np.random.RandomState(3)
    present = codes[rng.randint(0, len(codes), size=500_000)]
    present = np.where(rng.rand(len(present)) < 0.5, _rc(present, 21), present)
    other = rng.randint(0, 1 << 42, size=500_000, dtype=np.int64).astype(np.uint64)
    asked = np.concatenate([present, other])[rng.permutation(1_000_000)]
    canon = _canon(asked, 21)
    at = np.minimum(np.searchsorted(codes, canon), len(codes) - 1)
    want = np.where(codes[at] == canon, counts[at], 0).astype(np.int64)
    assert (want > 0).sum() >= 500_000
    assert np.array_equal(t.query(torch.from_numpy(asked.view(np.int64)).to(DEV)).cpu().numpy(), want)
    for high in (255, 10000):
        assert np.array_equal(t.spectrum(high), np.bincount(np.minimum(counts, high + 1).astype(np.int64), minlength=high + 2))


def test_a_pending_deferred_count_refuses():
    cfg = synth.SynthConfig(n_pairs=800, n_barcodes=11, n_genomes=2, genome_len=20_000, fragment=5_000, seed=51)
    s = synth.generate(cfg, device=DEV)
    t = kmer.KmerTable.with_slots(21, DEV, 20, 10)
    t.count(s, deferred_group=1)
    assert t.pending
    with pytest.raises(RuntimeError, match="deferred form"):
        t.query(np.zeros(3, np.uint64))
    with pytest.raises(RuntimeError, match="deferred form"):
        t.spectrum()


# ------------------------------------------------------------------------------------------------------------ the tool

def _histo_text(counts, high, full=False):
    hist = np.bincount(np.minimum(np.asarray(counts).astype(np.int64), high + 1), minlength=high + 2)
    return "".join(f"{c} {hist[c]}\n" for c in range(1, high + 2) if full or hist[c])


def _tool(*argv):
    try:
        return cli.main_kmer_table([str(a) for a in argv])
    except SystemExit as e:
        return e.code


def test_kmer_table_tool_on_goldens(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("PANGAEA_LOWERCASE_IS_BASE", raising=False)
    k = 15
    fq, dump = os.path.join(GOLDEN, "stlfr.fq"), os.path.join(GOLDEN, "stlfr.k15.dump")
    ocodes, ocounts = oracle.Table(k).count(oracle.Reads(fq).all_seq(), lowercase_is_base=True).items()
    out = tmp_path / "reads.histo"
    assert _tool("histo", "-i", fq, "-k", k, "-o", out) == 0
    assert out.read_text() == _histo_text(ocounts, 10000) and len(ocodes) > 0
    assert _tool("histo", "-i", fq, "-k", k, "--high", 3, "--full", "-o", out) == 0
    assert out.read_text() == _histo_text(ocounts, 3, full=True) and out.read_text().count("\n") == 4
    dcodes, dcounts = cli.load_dump(dump, k)
    assert _tool("histo", "-g", dump, "-k", k, "-o", out) == 0
    assert out.read_text() == _histo_text(dcounts, 10000)
    capsys.readouterr()
    # three k-mers of the dump (one asked by its other strand, one from a file) and one that is not in it
    have = set(dcodes.tolist())
    absent = next(int(c) for c in _canon(np.arange(1 << 12, dtype=np.uint64), k) if int(c) not in have)
    picks = [0, len(dcodes) // 2, len(dcodes) - 1]
    asked = _strings(dcodes[picks[:1]], k) + _strings(np.array([absent], np.uint64), k) + _strings(_rc(dcodes[picks[1:2]], k), k)
    qfile = tmp_path / "more.txt"
    qfile.write_text(_strings(dcodes[picks[2:]], k)[0] + "\n")
    want = [int(dcounts[picks[0]]), 0, int(dcounts[picks[1]]), int(dcounts[picks[2]])]
    assert _tool("query", "-g", dump, "-k", k, "-q", qfile, *asked) == 0
    got = capsys.readouterr().out
    assert got == "".join(f"{s} {c}\n" for s, c in zip(asked + [qfile.read_text().strip()], want))
    assert _tool("query", "-i", fq, "-k", k, *asked[:1]) == 0
    assert capsys.readouterr().out == f"{asked[0]} {int(ocounts[np.searchsorted(ocodes, _canon(kmer.encode_kmers(asked[:1], k), k)[0])])}\n"
    # soft-masked reads: the table follows jellyfish's rule as Feature applies it -- lower-case bases count
    soft = os.path.join(GOLDEN, "soft.fq")
    lenient = kmer.count_kmers(ReadStream.from_fastq(soft, device=DEV), k, lowercase_is_base=True)
    assert _tool("histo", "-i", soft, "-k", k, "-o", out) == 0
    assert out.read_text() == _histo_text(lenient.items()[1], 10000)
    assert out.read_text() == _histo_text(oracle.Table.from_dump(os.path.join(GOLDEN, "soft.k15.dump"), k).items()[1], 10000)
    monkeypatch.setenv("PANGAEA_LOWERCASE_IS_BASE", "0")
    strict = kmer.count_kmers(ReadStream.from_fastq(soft, device=DEV), k, lowercase_is_base=False)
    assert _tool("histo", "-i", soft, "-k", k, "-o", out) == 0
    assert out.read_text() == _histo_text(strict.items()[1], 10000)
