"""Summing finished tables: ``KmerTable.merged`` / ``KmerTable.add_table`` (pg_table_merge_aligned, pg_table_merge) and
``kmer_table merge`` -- what `jellyfish merge` gives over the tables of src/feature.py:76-94.

Integer results, compared exactly.  The expected table always comes from the oracle: ``oracle.Table(k).count(text).items()`` of
each input, summed in numpy with the destination kind's rule (``min(a + b, 2^21)`` for the packed kinds, the plain sum for dense
and the planes).  Two texts per k, cut from two synthetic read sets of different genomes: A is the first set, B the second half
of A followed by as much of the second set -- so the two share k-mers and each has its own (asserted on the oracle's items before
anything runs on the GPU)."""
import ctypes as C
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
PACKED = ("hash", "mini")

# (kind, k, log2_slots, log2_bucket): the cases of test_table_inspect_gpu.py -- every kind, the edges of its k range, tables with
# one bucket (2^14 slots: 128 KiB of LDS in the aligned form) and with thousands
CASES = [("dense", 4, 0, 0), ("dense", 8, 0, 0),
         ("hash", 11, 12, 0), ("hash", 21, 20, 10),
         ("wide", 22, 20, 0), ("wide", 31, 20, 0),
         ("mini", 13, 18, 12), ("mini", 15, 20, 10), ("mini", 21, 22, 10), ("mini", 21, 14, 14),
         ("miniw", 22, 20, 13), ("miniw", 31, 20, 13)]
_IDS = [f"{c[0]}-k{c[1]}-s{c[2]}-b{c[3]}" for c in CASES]
ALIGNED = [c for c in CASES if c[0] == "mini" or (c[0] == "hash" and c[3])]
CROSS = [("hash", "mini", 15), ("mini", "hash", 15), ("hash", "mini", 21), ("mini", "hash", 21), ("dense", "hash", 11), ("hash", "dense", 11),
         ("wide", "miniw", 25), ("miniw", "wide", 25),
         # the other ordered pairs of distinct kinds that share a k, each at the smallest k both admit (dense at k = 13: 256 MiB)
         ("dense", "wide", 11), ("wide", "dense", 11), ("dense", "mini", 13), ("mini", "dense", 13),
         ("hash", "wide", 15), ("wide", "hash", 15), ("mini", "wide", 15), ("wide", "mini", 15)]


def _rc(codes, k):
    c = np.asarray(codes, dtype=np.uint64).copy()
    out = np.zeros_like(c)
    for _ in range(k):
        out = (out << np.uint64(2)) | ((c & np.uint64(3)) ^ np.uint64(2))
        c >>= np.uint64(2)
    return out


def _chars(k, log2_slots):
    """characters of text A (and of B): few enough for the smallest table of the case, and -- for k = 4 and 8 -- for a text
    that does not hold nearly every k-mer there is"""
    if k == 4:
        return 64
    if k == 8:
        return 6_000
    if log2_slots == 12:
        return 2_400                     # hash, 2^12 slots, unbucketed: A and B each fill it about half
    if log2_slots == 14:
        return 7_200                     # one bucket of 2^14 slots that must hold the union
    return 150_000                       # 500 read pairs


@functools.lru_cache(maxsize=None)
def _texts(k, n_chars):
    """(text A, text B, items of A, items of B) -- the sharing the tests rest on is asserted here, on the oracle alone"""
    sets = []
    for seed in (500 + k, 900 + k):
        cfg = synth.SynthConfig(n_pairs=max(2, n_chars // 300 + 1), n_barcodes=3, n_genomes=3, genome_len=30_000, fragment=8_000, sub_rate=0.01,
                                n_rate=0.2, seed=seed)
        sets.append(synth.generate(cfg, device="cpu").decode()[:n_chars])
    a = sets[0] + b"N"
    b = sets[0][n_chars // 2:] + b"N" + sets[1][:n_chars // 2] + b"N"
    ia, ib = (oracle.Table(k, threads=4).count(t).items() for t in (a, b))
    shared = np.isin(ib[0], ia[0]).sum()
    assert len(ib[0]) >= 16 and 4 * shared >= len(ib[0]) and 4 * (len(ib[0]) - shared) >= len(ib[0]), (k, len(ia[0]), len(ib[0]), shared)
    return a, b, ia, ib


def _expected(items, packed):
    """the sum of several (codes, counts), with the destination kind's rule"""
    codes = np.concatenate([np.asarray(c, dtype=np.uint64) for c, _ in items])
    counts = np.concatenate([np.minimum(np.asarray(n).astype(np.int64), SAT) if packed else np.asarray(n).astype(np.int64) for _, n in items])
    u, inv = np.unique(codes, return_inverse=True)
    total = np.zeros(len(u), np.int64)
    np.add.at(total, inv, counts)
    return u, np.minimum(total, SAT) if packed else total


def _fresh(kind, k, log2_slots, log2_bucket):
    if kind == "dense":
        return kmer.KmerTable.alloc(k, DEV, "dense")
    if kind == "hash":
        return kmer.KmerTable.with_slots(k, DEV, log2_slots, log2_bucket)
    if kind == "wide":
        return kmer.KmerTable.wide_with_slots(k, DEV, log2_slots)
    return kmer.KmerTable.mini_with_slots(k, DEV, log2_slots, log2_bucket)


def _counted(case, text):
    t = _fresh(*case).count(ReadStream.from_runs([("a", text)], device=DEV))
    assert t.kind == case[0]
    return t


@functools.lru_cache(maxsize=None)
def _pair(case):
    """(table A, table B, items of A, items of B) of a case; the tables are only ever read"""
    a, b, ia, ib = _texts(case[1], _chars(case[1], case[2]))
    return _counted(case, a), _counted(case, b), ia, ib


def _applies(a, b):
    return _lib.load().pg_table_merge_aligned_applies(a.desc(), b.desc()) == 1


def _holds(t, want, k=None):
    """the table holds exactly ``want`` = (codes, counts): by items(), by query() on both strands, by spectrum()"""
    codes, counts = t.items()
    assert np.array_equal(codes, want[0]) and np.array_equal(counts.astype(np.int64), want[1])
    if k is not None:
        assert np.array_equal(t.query(want[0]).cpu().numpy(), want[1])
        assert np.array_equal(t.query(_rc(want[0], k)).cpu().numpy(), want[1])
        assert np.array_equal(t.spectrum(255), np.bincount(np.minimum(want[1], 256), minlength=257))


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_same_kind_every_kind(case):
    kind, k = case[0], case[1]
    A, B, ia, ib = _pair(case)
    before = A.data.clone(), B.data.clone()
    m = kmer.KmerTable.merged([A, B])
    assert m.kind == kind and m.k == k and m is not A and m is not B
    _holds(m, _expected([ia, ib], kind in PACKED), k)
    assert _applies(A, B) == (case in ALIGNED)
    assert m.merge_form == ("aligned" if case in ALIGNED else "general")
    if case in ALIGNED:
        assert (m.log2_slots, m.log2_bucket) == (A.log2_slots, A.log2_bucket)
    assert torch.equal(A.data, before[0]) and torch.equal(B.data, before[1])


@pytest.mark.parametrize("case", ALIGNED, ids=[_IDS[CASES.index(c)] for c in ALIGNED])
def test_aligned_and_general_agree(case):
    A, B, ia, ib = _pair(case)
    m = kmer.KmerTable.merged([A, B])
    assert m.merge_form == "aligned"
    g = _fresh(*case).add_table(A).add_table(B)
    assert all(np.array_equal(x, y) for x, y in zip(g.items(), m.items()))
    _holds(g, _expected([ia, ib], True), case[1])


@pytest.mark.parametrize("src,dst,k", CROSS, ids=[f"{s}-to-{d}-k{k}" for s, d, k in CROSS])
def test_cross_kind(src, dst, k):
    assert kmer.KmerTable.kind_admits(src, k) and kmer.KmerTable.kind_admits(dst, k)
    a, b, ia, ib = _texts(k, 60_000)
    A = kmer.count_kmers(ReadStream.from_runs([("a", a)], device=DEV), k, kind=src)
    B = kmer.count_kmers(ReadStream.from_runs([("b", b)], device=DEV), k, kind=dst)
    assert (A.kind, B.kind) == (src, dst)
    before = A.data.clone(), B.data.clone()
    m = kmer.KmerTable.merged([A, B], kind=dst)                       # sources of two kinds into one destination
    assert m.kind == dst and m.merge_form == "general"
    _holds(m, _expected([ia, ib], dst in PACKED), k)
    m = kmer.KmerTable.merged([B, A, B], kind=src)
    assert m.kind == src and m.merge_form == "general"
    _holds(m, _expected([ib, ia, ib], src in PACKED), k)
    assert torch.equal(A.data, before[0]) and torch.equal(B.data, before[1])


def test_union_larger_than_the_geometry():
    k, case = 21, ("mini", 21, 14, 14)
    texts = []
    for seed in (71, 72):
        cfg = synth.SynthConfig(n_pairs=50, n_barcodes=2, n_genomes=3, genome_len=30_000, fragment=8_000, sub_rate=0.01, n_rate=0.2, seed=seed)
        texts.append(synth.generate(cfg, device="cpu").decode()[:12_800] + b"N")
    ia, ib = (oracle.Table(k, threads=4).count(t).items() for t in texts)
    assert max(len(ia[0]), len(ib[0])) <= 0.6 * (1 << 14) and len(np.union1d(ia[0], ib[0])) > (1 << 14), (len(ia[0]), len(ib[0]))
    A, B = _counted(case, texts[0]), _counted(case, texts[1])
    assert _applies(A, B)
    m = kmer.KmerTable.merged([A, B])
    assert m.merge_form == "general" and m.kind == "mini" and m.log2_slots > 14
    _holds(m, _expected([ia, ib], True), k)
    # the aligned form itself, on the same inputs: a full bucket is a status bit, not a fault
    dst = kmer.KmerTable.mini_with_slots(k, DEV, 14, 14)
    srcs = (C.POINTER(_lib.pg_table) * 2)(C.pointer(A._desc), C.pointer(B._desc))
    with torch.cuda.device(dst.device):
        rc = _lib.load().pg_table_merge_aligned(dst.desc(), srcs, 2, dst.status.data_ptr(), kmer._stream_ptr(dst.device))
    torch.cuda.synchronize()
    assert rc == 0 and int(dst.status[0].item()) & _lib.STATUS_TABLE_FULL


def _some_codes(k, n, seed):
    """n canonical k-mers, sorted"""
    raw = np.random.RandomState(seed).randint(0, 1 << 62, size=4 * n, dtype=np.int64).astype(np.uint64) & np.uint64((1 << (2 * k)) - 1)
    return np.unique(np.minimum(raw, _rc(raw, k)))[:n]


def _items_table(kind, k, codes, counts, geometry=None):
    codes, counts = np.asarray(codes, dtype=np.uint64), np.asarray(counts, dtype=np.uint64)
    if geometry is None:
        return kmer.KmerTable.from_items(k, codes, counts, DEV, kind)
    t = kmer.KmerTable.with_slots(k, DEV, *geometry)                  # a bucketed hash table
    return t.merge(torch.from_numpy(((kmer.key42(codes) << np.uint64(22)) | counts).view(np.int64)))


@pytest.mark.parametrize("kind,geometry", [("mini", None), ("hash", None), ("hash", (14, 10))])
def test_saturation_of_the_packed_kinds(kind, geometry):
    k = 21
    c = _some_codes(k, 5, 1)
    A = _items_table(kind, k, c[:4], [SAT - 1, SAT, 7, SAT - 3], geometry)
    B = _items_table(kind, k, c[[0, 1, 3, 4]], [5, SAT, 3, 9], geometry)
    want = (c, np.array([SAT, SAT, 7, SAT, 9], dtype=np.int64))
    m = kmer.KmerTable.merged([A, B])
    assert m.merge_form == ("aligned" if _applies(A, B) else "general") and (kind == "mini" or geometry is not None) == _applies(A, B)
    _holds(m, want, k)
    _holds(kmer.KmerTable.alloc(k, DEV, kind).add_table(A).add_table(B), want, k)


@pytest.mark.parametrize("kind", ["wide", "miniw"])
def test_the_planes_sum_in_32_bits_and_carry_a_packed_source(kind):
    k = 25
    c = _some_codes(k, 3, 2)
    A = _items_table(kind, k, c[:2], [6_000_000, 4])
    B = _items_table(kind, k, c[[0, 2]], [6_000_000, 1])
    _holds(kmer.KmerTable.merged([A, B]), (c, np.array([12_000_000, 4, 1], dtype=np.int64)), k)
    # a packed source's saturated count travels as the value it stores
    k = 21
    c = _some_codes(k, 2, 3)
    P = _items_table("mini", k, c, [3 * SAT, 10])
    W = _items_table("wide", k, c[:1], [6_000_000])
    assert P.items()[1].tolist() == [SAT, 10]
    m = kmer.KmerTable.merged([P, W], kind="wide")
    _holds(m, (c, np.array([SAT + 6_000_000, 10], dtype=np.int64)), k)
    m = kmer.KmerTable.merged([W, P, W], kind="mini")                 # ... and a wide count enters a packed table clamped
    _holds(m, (c, np.array([SAT, 10], dtype=np.int64)), k)


@pytest.mark.parametrize("case", [("mini", 15, 20, 10), ("hash", 21, 20, 10), ("wide", 22, 20, 0), ("dense", 8, 0, 0)], ids=lambda c: c[0])
def test_degenerate_shapes(case):
    kind, k = case[0], case[1]
    A, B, ia, ib = _pair(case)
    packed = kind in PACKED
    before = A.data.clone(), B.data.clone()
    _holds(kmer.KmerTable.merged([A, B, A]), _expected([ia, ib, ia], packed), k)
    one = kmer.KmerTable.merged([A])
    assert one is not A and one.data.data_ptr() != A.data.data_ptr()
    _holds(one, _expected([ia], packed), k)
    _holds(kmer.KmerTable.merged([A, A]), _expected([ia, ia], packed), k)
    empty = _fresh(*case)
    _holds(kmer.KmerTable.merged([A, empty]), _expected([ia], packed), k)
    _holds(kmer.KmerTable.merged([empty, A, empty]), _expected([ia], packed), k)
    assert len(kmer.KmerTable.merged([empty, empty]).items()[0]) == 0
    if case[3]:                                                       # a reset() bucketed table is empty whatever its memory holds
        gone = _counted(case, _texts(k, _chars(k, case[2]))[1]).reset()
        m = kmer.KmerTable.merged([gone, A])
        assert m.merge_form == "aligned"
        _holds(m, _expected([ia], packed), k)
        _holds(_fresh(*case).add_table(gone).add_table(A), _expected([ia], packed), k)
    assert torch.equal(A.data, before[0]) and torch.equal(B.data, before[1])


def test_refusals_come_before_any_launch():
    A, B, ia, ib = _pair(("mini", 21, 22, 10))
    other_k = _pair(("mini", 15, 20, 10))[0]
    before = A.data.clone(), B.data.clone(), other_k.data.clone()
    with pytest.raises(ValueError, match="different k"):
        kmer.KmerTable.merged([A, other_k])
    with pytest.raises(ValueError, match="different k"):
        A.add_table(other_k)
    for bad in ("dense", "miniw", "no such kind"):
        with pytest.raises(ValueError, match="do not admit k = 21"):
            kmer.KmerTable.merged([A, B], kind=bad)
    with pytest.raises(ValueError, match="itself"):
        A.add_table(A)
    with pytest.raises(ValueError, match="at least one table"):
        kmer.KmerTable.merged([])
    with pytest.raises(TypeError):
        A.add_table(A.data)
    cfg = synth.SynthConfig(n_pairs=800, n_barcodes=11, n_genomes=2, genome_len=20_000, fragment=5_000, seed=51)
    pending = kmer.KmerTable.with_slots(21, DEV, 20, 10)
    pending.count(synth.generate(cfg, device=DEV), deferred_group=1)
    assert pending.pending
    for call in (lambda: kmer.KmerTable.merged([A, pending]), lambda: kmer.KmerTable.merged([pending, A]), lambda: A.add_table(pending),
                 lambda: pending.add_table(A)):
        with pytest.raises(RuntimeError, match="deferred form"):
            call()
    assert torch.equal(A.data, before[0]) and torch.equal(B.data, before[1]) and torch.equal(other_k.data, before[2])
    _holds(A, _expected([ia], True))


GUARD = 4096                      # 8-byte words in front of and behind the destination
PATTERN = 0x5A5A_1234_5A5A_4321


@pytest.mark.parametrize("case", [("mini", 15, 20, 10), ("mini", 21, 14, 14), ("hash", 21, 20, 10), ("miniw", 22, 20, 13), ("dense", 8, 0, 0)],
                         ids=lambda c: f"{c[0]}-s{c[2]}-b{c[3]}")
def test_nothing_is_stored_outside_the_destination(case):
    """the destination is a view inside a larger tensor filled with a pattern; both forms, a table of many buckets and one of a
    single bucket: the words around the view keep the pattern"""
    kind, k = case[0], case[1]
    A, B, ia, ib = _pair(case)
    want = _expected([ia, ib], kind in PACKED)
    big = torch.full((GUARD + A.data.numel() * A.data.element_size() // 8 + GUARD,), PATTERN, dtype=torch.int64, device=DEV)
    view = big[GUARD:-GUARD].view(A.data.dtype)
    forms = ("aligned", "general") if case in ALIGNED else ("general",)
    for form in forms:
        big.fill_(PATTERN)
        dst = kmer.KmerTable(k, kind, view, A.log2_slots, A.log2_bucket)
        if form == "aligned":                                         # (the old slice is neither read nor cleared)
            srcs = (C.POINTER(_lib.pg_table) * 2)(C.pointer(A._desc), C.pointer(B._desc))
            with torch.cuda.device(dst.device):
                _lib.check(_lib.load().pg_table_merge_aligned(dst.desc(), srcs, 2, dst.status.data_ptr(), kmer._stream_ptr(dst.device)))
            dst._empty = False
            dst.check_status()
        else:
            view.zero_()
            dst.add_table(A).add_table(B)
        _holds(dst, want, k)
        assert bool((big[:GUARD] == PATTERN).all()) and bool((big[-GUARD:] == PATTERN).all()), form


# ------------------------------------------------------------------------------------------------------------ the tool

def _tool(*argv):
    try:
        return cli.main_kmer_table([str(a) for a in argv])
    except SystemExit as e:
        return e.code


def _g(name):
    return os.path.join(GOLDEN, name)


def test_kmer_table_merge_on_goldens(tmp_path, monkeypatch):
    monkeypatch.delenv("PANGAEA_LOWERCASE_IS_BASE", raising=False)
    out = tmp_path / "merged.dump"
    k, names = 15, ("pair.k15.dump", "pairq.k15.dump", "soft.k15.dump")
    want = _expected([cli.load_dump(_g(n), k) for n in names], True)
    assert len(want[0]) > 100 and want[1].max() >= 2
    assert _tool("merge", "-k", k, "-g", _g(names[0]), "-g", _g(names[1]), "-g", _g(names[2]), "-o", out) == 0
    got = cli.load_dump(str(out), k)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].astype(np.int64), want[1])
    assert _tool("merge", "-k", k, "-g", _g(names[0]), "-g", _g(names[1]), "-g", _g(names[2]), "-L", 2, "-o", out) == 0
    got = cli.load_dump(str(out), k)
    keep = want[1] >= 2
    assert 0 < keep.sum() < len(keep)
    assert np.array_equal(got[0], want[0][keep]) and np.array_equal(got[1].astype(np.int64), want[1][keep])
    # one pair at k = 21
    k, names = 21, ("soft.k21.dump", "tenx_clean.k21.dump")
    want = _expected([cli.load_dump(_g(n), k) for n in names], True)
    assert _tool("merge", "-k", k, "-g", _g(names[0]), "-g", _g(names[1]), "-o", out) == 0
    got = cli.load_dump(str(out), k)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].astype(np.int64), want[1])
    # reads and a dump: the oracle's count of the reads (jellyfish's rule: lower-case bases count) plus the dump
    k = 15
    counted = oracle.Table(k).count(oracle.Reads(_g("soft.fq")).all_seq(), lowercase_is_base=True).items()
    want = _expected([counted, cli.load_dump(_g("soft.k15.dump"), k)], True)
    assert _tool("merge", "-k", k, "-i", _g("soft.fq"), "-g", _g("soft.k15.dump"), "-o", out) == 0
    got = cli.load_dump(str(out), k)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].astype(np.int64), want[1])
