"""Two finished tables met otherwise than by their sum: ``KmerTable.combined`` / ``filtered`` / ``compare``
(pg_table_combine_aligned, pg_table_combine_items, pg_table_compare) and ``kmer_table combine | compare | dump -U``.

Integer results, compared exactly.  The expected items always come from the oracle: ``oracle.Table(k).count(text).items()`` of each
input, clamped to HASH_COUNT_SAT where the kind that stores them is packed, combined in numpy with the rule of the op --
min(a, b); max(a, b); a - b where a > b; a where b > 0; a where b == 0; a -- cut to lower <= r <= upper and clamped again where the
result's kind is packed.  The texts, tables and cases are those of test_table_merge_gpu.py (A, and B = the second half of A + as much
of another genome set: at least a quarter shared, at least a quarter own, asserted there on the oracle's items)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from pangaea_amd import _lib, cli, kmer, synth
from pangaea_amd.reads import ReadStream

from . import test_mini_find_gpu as find
from . import test_table_merge_gpu as merge
from .conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAT = _lib.HASH_COUNT_SAT
PACKED = ("hash", "mini")
OPS = ("min", "max", "diff", "left", "only")
CASES, ALIGNED, CROSS = merge.CASES, merge.ALIGNED, merge.CROSS
_IDS = merge._IDS


def _expected(ia, ib, op, packed_a=False, packed_b=False, packed_out=False, lower=1, upper=None):
    """(codes, counts) the result must hold; ``ib`` None for ``keep``"""
    if ib is None:
        ib = (np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    codes = np.union1d(np.asarray(ia[0], dtype=np.uint64), np.asarray(ib[0], dtype=np.uint64))
    a, b = np.zeros(len(codes), np.int64), np.zeros(len(codes), np.int64)
    a[np.searchsorted(codes, np.asarray(ia[0], dtype=np.uint64))] = np.asarray(ia[1]).astype(np.int64)
    b[np.searchsorted(codes, np.asarray(ib[0], dtype=np.uint64))] = np.asarray(ib[1]).astype(np.int64)
    if packed_a:
        a = np.minimum(a, SAT)
    if packed_b:
        b = np.minimum(b, SAT)
    r = {"min": np.minimum(a, b), "max": np.maximum(a, b), "diff": np.where(a > b, a - b, 0), "left": np.where(b > 0, a, 0),
         "only": np.where(b == 0, a, 0), "keep": a}[op]
    keep = (r >= lower) & (r > 0)
    if upper is not None:
        keep &= r <= upper
    r = np.minimum(r, SAT) if packed_out else r
    return codes[keep], r[keep]


def _holds(t, want, k):
    merge._holds(t, want, k)
    assert int(t.status[0].item()) == 0


def _empty(t, probes, tmp_path=None):
    assert len(t.items()[0]) == 0 and not t.query(probes).any() and not t.spectrum(255).any()
    if tmp_path is not None:
        path = tmp_path / "empty.dump"
        assert t.write_dump(str(path))[0] == 0 and os.path.getsize(path) == 0


# 1 ---- every kind, every op, same kind
@pytest.mark.parametrize("op", OPS + ("keep",))
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_same_kind_every_kind(case, op):
    kind, k = case[0], case[1]
    A, B, ia, ib = merge._pair(case)
    before = A.data.clone(), B.data.clone()
    packed = kind in PACKED
    if op == "keep":
        r = A.filtered()
        want = _expected(ia, None, op, packed, packed, packed)
    else:
        r = kmer.KmerTable.combined(A, B, op)
        want = _expected(ia, ib, op, packed, packed, packed)
    assert r.kind == kind and r.k == k and r is not A and r is not B and len(want[0]) > 0
    _holds(r, want, k)
    assert r.combine_form == ("aligned" if case in ALIGNED else "general")
    if case in ALIGNED:
        assert (r.log2_slots, r.log2_bucket) == (A.log2_slots, A.log2_bucket)
    assert torch.equal(A.data, before[0]) and torch.equal(B.data, before[1])


# ... and the two forms agree on the tables the aligned form takes (the general one asked for through the entry itself)
@pytest.mark.parametrize("case", ALIGNED, ids=[_IDS[CASES.index(c)] for c in ALIGNED])
def test_items_of_the_general_form_on_aligned_tables(case):
    k = case[1]
    A, B, ia, ib = merge._pair(case)
    L = _lib.load()
    cap = len(ia[0])
    for op in OPS:
        codes = torch.empty(cap, dtype=torch.int64, device=DEV)
        counts = torch.empty(cap, dtype=torch.int32, device=DEV)
        n_out = torch.zeros(1, dtype=torch.int64, device=DEV)
        status = torch.zeros(2, dtype=torch.int32, device=DEV)
        with torch.cuda.device(A.device):
            _lib.check(L.pg_table_combine_items(A.desc(), B.desc(), _lib.COMBINE_OPS[op], 1, -1, codes.data_ptr(), counts.data_ptr(), cap,
                                                n_out.data_ptr(), status.data_ptr(), kmer._stream_ptr(A.device)))
        n = int(n_out.item())
        assert int(status[0].item()) == 0 and n <= cap
        # (max over A's entries only: the rest of the union is the second launch's)
        want = _expected(ia, ib, op, True, True) if op != "max" else _expected(ia, (ib[0], ib[1]), "max", True, True)
        if op == "max":
            mine = np.isin(want[0], ia[0])
            want = want[0][mine], want[1][mine]
        order = np.argsort(codes[:n].cpu().numpy().view(np.uint64))
        assert np.array_equal(codes[:n].cpu().numpy().view(np.uint64)[order], want[0])
        assert np.array_equal(counts[:n].cpu().numpy().astype(np.int64)[order], want[1])


def test_items_past_the_capacity_are_not_stored():
    case = ("mini", 15, 20, 10)
    A, B, ia, ib = merge._pair(case)
    want = _expected(ia, ib, "left", True, True)
    cap = len(want[0]) // 2
    guard = 64
    codes = torch.full((cap + guard,), -7, dtype=torch.int64, device=DEV)
    counts = torch.full((cap + guard,), -7, dtype=torch.int32, device=DEV)
    n_out = torch.zeros(1, dtype=torch.int64, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    with torch.cuda.device(A.device):
        _lib.check(_lib.load().pg_table_combine_items(A.desc(), B.desc(), _lib.COMBINE_LEFT, 1, -1, codes.data_ptr(), counts.data_ptr(), cap,
                                                      n_out.data_ptr(), status.data_ptr(), kmer._stream_ptr(A.device)))
    assert int(n_out.item()) == len(want[0]) and int(status[0].item()) == _lib.STATUS_OVERFLOW_LIST
    assert bool((codes[cap:] == -7).all()) and bool((counts[cap:] == -7).all())
    got = codes[:cap].cpu().numpy().view(np.uint64)
    assert len(np.unique(got)) == cap and np.isin(got, want[0]).all()


# 2 ---- cross kinds and kind=
@functools.lru_cache(maxsize=None)
def _cross_pair(src, dst, k):
    a, b, ia, ib = merge._texts(k, 60_000)
    A = kmer.count_kmers(ReadStream.from_runs([("a", a)], device=DEV), k, kind=src)
    B = kmer.count_kmers(ReadStream.from_runs([("b", b)], device=DEV), k, kind=dst)
    assert (A.kind, B.kind) == (src, dst)
    return A, B, ia, ib


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("src,dst,k", CROSS, ids=[f"{s}-x-{d}-k{k}" for s, d, k in CROSS])
def test_cross_kind(src, dst, k, op):
    assert kmer.KmerTable.kind_admits(src, k) and kmer.KmerTable.kind_admits(dst, k)
    A, B, ia, ib = _cross_pair(src, dst, k)
    before = A.data.clone(), B.data.clone()
    r = kmer.KmerTable.combined(A, B, op)                                # the result takes A's kind ...
    assert r.kind == src and r.combine_form == "general"
    _holds(r, _expected(ia, ib, op, src in PACKED, dst in PACKED, src in PACKED), k)
    r = kmer.KmerTable.combined(A, B, op, kind=dst)                      # ... or the one named
    assert r.kind == dst and r.combine_form == "general"
    _holds(r, _expected(ia, ib, op, src in PACKED, dst in PACKED, dst in PACKED), k)
    assert torch.equal(A.data, before[0]) and torch.equal(B.data, before[1])


def test_kind_of_same_kind_sources_takes_the_general_form():
    case = ("mini", 21, 22, 10)
    A, B, ia, ib = merge._pair(case)
    r = kmer.KmerTable.combined(A, B, "diff", kind="hash")
    assert r.kind == "hash" and r.combine_form == "general"
    _holds(r, _expected(ia, ib, "diff", True, True, True), 21)
    r = A.filtered(2, None, kind="wide")
    assert r.kind == "wide" and r.combine_form == "general"
    _holds(r, _expected(ia, None, "keep", True, lower=2), 21)


# 3 ---- empty and total results
@functools.lru_cache(maxsize=None)
def _disjoint_texts(k, n_chars=60_000):
    a, c = find._text(find._runs(500 + k))[:n_chars] + b"N", find._text(find._runs(900 + k))[:n_chars] + b"N"
    ia, ic = (oracle.Table(k, threads=4).count(t).items() for t in (a, c))
    assert len(ia[0]) > 1000 and len(ic[0]) > 1000 and not np.isin(ia[0], ic[0]).any()
    return a, c, ia, ic


EDGE_CASES = [("mini", 21, 20, 10), ("hash", 21, 20, 10)]


@functools.lru_cache(maxsize=None)
def _disjoint_pair(case):
    a, c, ia, ic = _disjoint_texts(case[1])
    return merge._counted(case, a), merge._counted(case, c), ia, ic


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: c[0])
def test_nothing_shared(case, tmp_path):
    k = case[1]
    A, Cc, ia, ic = _disjoint_pair(case)
    probes = np.concatenate([ia[0], ic[0]])
    for op in ("min", "left"):
        r = kmer.KmerTable.combined(A, Cc, op)
        assert r.combine_form == "aligned"
        _empty(r, probes, tmp_path)
    for op in ("only", "diff"):
        r = kmer.KmerTable.combined(A, Cc, op)
        assert r.combine_form == "aligned"
        _holds(r, _expected(ia, None, "keep", True), k)
    r = kmer.KmerTable.combined(A, Cc, "max")
    assert r.combine_form == "aligned"
    want = _expected(ia, ic, "max", True, True, True)
    assert len(want[0]) == len(ia[0]) + len(ic[0])
    _holds(r, want, k)


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: c[0])
def test_a_table_against_itself(case, tmp_path):
    k = case[1]
    A, _, ia, _ = _disjoint_pair(case)
    before = A.data.clone()
    for op in ("diff", "only"):
        r = kmer.KmerTable.combined(A, A, op)
        assert r.combine_form == "aligned"
        _empty(r, ia[0], tmp_path)
    for op in ("min", "max", "left"):
        r = kmer.KmerTable.combined(A, A, op)
        assert r.combine_form == "aligned" and r.data.data_ptr() != A.data.data_ptr()
        _holds(r, _expected(ia, None, "keep", True), k)
    assert torch.equal(A.data, before)


# 4 ---- crowded buckets: removing entries from chains that run through most of a bucket -- the rebuild
@functools.lru_cache(maxsize=None)
def _crowded_texts():
    k, log2_slots = 21, 13
    text_a, text_c = find._text(find._runs(500 + k)), find._text(find._runs(900 + k))
    # the text length with the oracle, as test_crowded_buckets finds it: read pairs until the table holds 0.62 x 2^13 distinct k-mers
    otab, n_chars = oracle.Table(k), 0
    while len(otab) < 0.62 * (1 << log2_slots):
        otab.count(text_a[n_chars:n_chars + 302])
        n_chars += 302
    assert n_chars < len(text_a) and len(otab) <= 0.7 * (1 << log2_slots)
    a = text_a[:n_chars]
    b = text_a[n_chars // 2 // 302 * 302:n_chars] + text_c[:n_chars // 4 // 302 * 302]
    ia, ib = (oracle.Table(k, threads=4).count(t).items() for t in (a, b))
    assert 0.25 <= np.isin(ia[0], ib[0]).mean() <= 0.75 and len(ib[0]) <= 0.7 * (1 << log2_slots)
    return a, b, ia, ib


@pytest.mark.parametrize("kind", ["mini", "hash"])
def test_crowded_buckets_are_rebuilt(kind):
    k, log2_slots, log2_bucket = 21, 13, 10
    a, b, ia, ib = _crowded_texts()
    tables = []
    for text in (a, b):
        src = kmer.count_kmers(find._stream([("t", text)]), k, kind="hash")
        t = merge._fresh(kind, k, log2_slots, log2_bucket)
        t.add_table(src)
        tables.append(t)
    A, B = tables
    fill = (A.data.view(A.n_buckets, -1) != 0).sum(dim=1).cpu().numpy()
    assert fill.sum() == len(ia[0]) and fill.sum() >= 0.6 * (1 << log2_slots) and fill.max() >= 0.6 * (1 << log2_bucket)
    before = A.data.clone(), B.data.clone()
    for op in ("only", "left", "diff"):
        r = kmer.KmerTable.combined(A, B, op)
        assert r.combine_form == "aligned"
        want = _expected(ia, ib, op, True, True, True)
        gone = np.setdiff1d(ia[0], want[0])
        assert len(want[0]) >= 0.1 * len(ia[0]) and len(gone) >= 0.1 * len(ia[0])
        _holds(r, want, k)                                             # (every survivor is found, on both strands)
        assert not r.query(gone).any() and not r.query(merge._rc(gone, k)).any()
    assert torch.equal(A.data, before[0]) and torch.equal(B.data, before[1])


# 5 ---- chosen counts, the window's edges
#        a: equal, b = a + 1, b = a - 1, 1 and 1, 1 and SAT - 1, SAT - 1 and SAT, SAT and SAT, SAT and 1, only in A (twice), only in B
PAIRS = [(5, 5), (7, 8), (8, 7), (1, 1), (1, SAT - 1), (SAT - 1, SAT), (SAT, SAT), (SAT, 1), (3, 0), (SAT - 1, 0), (0, 4), (0, SAT)]
WIDE_PAIRS = PAIRS + [(SAT + 1000, 5), (6_000_000, SAT + 7), (SAT + 1, SAT + 1), (0, 3 * SAT)]


def _chosen(kind, k, pairs):
    c = merge._some_codes(k, len(pairs), 11 + k)
    a, b = np.array([p[0] for p in pairs], dtype=np.uint64), np.array([p[1] for p in pairs], dtype=np.uint64)
    ia, ib = (c[a > 0], a[a > 0]), (c[b > 0], b[b > 0])
    return merge._items_table(kind, k, *ia), merge._items_table(kind, k, *ib), ia, ib


def _windows(values):
    """lower / upper exactly on, one below and one above each of the values"""
    out = [(1, None)]
    for v in values:
        out += [(v, None), (v + 1, None), (max(1, v - 1), None), (1, v), (1, v + 1), (v, v)] + ([(1, v - 1)] if v > 1 else [])
    return out


@pytest.mark.parametrize("kind,k", [("mini", 15), ("hash", 21), ("wide", 25)])
def test_chosen_counts_and_windows(kind, k):
    packed = kind in PACKED
    A, B, ia, ib = _chosen(kind, k, PAIRS if packed else WIDE_PAIRS)
    for op in OPS:
        for lower, upper in _windows((1, 7, SAT - 1, SAT)):
            r = kmer.KmerTable.combined(A, B, op, lower=lower, upper=upper)
            assert r.combine_form == ("aligned" if kind == "mini" else "general")
            want = _expected(ia, ib, op, packed, packed, packed, lower, upper)
            got = r.items()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].astype(np.int64), want[1]), (op, lower, upper)
    for lower, upper in _windows((3, 7, SAT - 1)):
        r = A.filtered(lower, upper)
        want = _expected(ia, None, "keep", packed, False, packed, lower, upper)
        got = r.items()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].astype(np.int64), want[1]), (lower, upper)
        stored = np.minimum(ia[1].astype(np.int64), SAT) if packed else ia[1].astype(np.int64)
        assert np.array_equal(r.query(ia[0]).cpu().numpy(), np.where(np.isin(ia[0], want[0]), stored, 0))


def test_a_wide_count_enters_a_packed_kind_clamped():
    k = 21
    A, B, ia, ib = _chosen("wide", k, WIDE_PAIRS)
    for op in OPS:
        for kind in PACKED:
            r = kmer.KmerTable.combined(A, B, op, kind=kind)
            assert r.kind == kind and r.combine_form == "general"
            want = _expected(ia, ib, op, False, False, True)
            assert want[1].max() <= SAT
            _holds(r, want, k)
    r = A.filtered(SAT + 1, None, kind="mini")                         # the window sees the stored count, the packed table its clamp
    want = _expected(ia, None, "keep", False, False, True, SAT + 1)
    assert len(want[0]) == 3 and (want[1] == SAT).all()
    _holds(r, want, k)


# 6 ---- a union that does not fit the geometry
UNION_CHARS = 12_800          # of each of the two genome sets: 8 184 and 9 026 distinct 21-mers, together more than the bucket's 2^14


def test_union_larger_than_the_geometry():
    k, case = 21, ("mini", 21, 14, 14)
    texts = []
    for seed in (71, 72):
        cfg = synth.SynthConfig(n_pairs=50, n_barcodes=2, n_genomes=3, genome_len=30_000, fragment=8_000, sub_rate=0.01, n_rate=0.2, seed=seed)
        texts.append(synth.generate(cfg, device="cpu").decode()[:UNION_CHARS] + b"N")
    ia, ib = (oracle.Table(k, threads=4).count(t).items() for t in texts)
    assert max(len(ia[0]), len(ib[0])) <= 0.6 * (1 << 14) and len(np.union1d(ia[0], ib[0])) > (1 << 14), (len(ia[0]), len(ib[0]))
    A, B = merge._counted(case, texts[0]), merge._counted(case, texts[1])
    assert merge._applies(A, B)
    r = kmer.KmerTable.combined(A, B, "max")
    assert r.combine_form == "general" and r.kind == "mini" and r.log2_slots > 14
    _holds(r, _expected(ia, ib, "max", True, True, True), k)
    assert not r.status.any()
    for op in ("min", "only"):                                       # the subset ops always fit
        r = kmer.KmerTable.combined(A, B, op)
        assert r.combine_form == "aligned"
        _holds(r, _expected(ia, ib, op, True, True, True), k)


# 7 ---- downstream: the rows of other reads against a combined and a filtered table, in the find form
@pytest.mark.parametrize("k", [15, 21])
def test_rows_against_combined_tables(k):
    a, c = find._runs(500 + k), find._runs(900 + k)
    b = find._second_half_plus(a, c)
    # B's table holds a part of B's reads only: some of B's k-mers that A holds stay in `only`, the others leave
    part = b[:len(b) // 4] + b[-(len(b) // 4):]
    ia, ib = (oracle.Table(k, threads=4).count(find._text(r)).items() for r in (a, part))
    A, B = find._mini(k, 20, 10, find._stream(a)), find._mini(k, 20, 10, find._stream(part))
    sb = find._stream(b)
    rows = sb.rows(302)
    plan = kmer.Plan(rows, DEV)
    for table, want_items in ((kmer.KmerTable.combined(A, B, "only"), _expected(ia, ib, "only", True, True, True)),
                              (A.filtered(2, None), _expected(ia, None, "keep", True, lower=2))):
        assert table.combine_form == "aligned" and 0 < len(want_items[0]) < len(ia[0])
        otab = oracle.Table(k)
        for code, n in zip(want_items[0].tolist(), want_items[1].tolist()):
            otab.set(code, n)
        assert 0.05 <= find._share(k, otab, find._text(b)) <= 0.95
        want = find._want(sb, rows, k, otab, 10, 400)
        assert want.sum() > 0
        assert np.array_equal(find._rows(table, sb, plan), want)       # (asserts rows_form == "find")


# 8 ---- compare
def _compared(ia, ib, packed_a, packed_b):
    a, b = (np.minimum(np.asarray(n).astype(np.int64), SAT) if p else np.asarray(n).astype(np.int64) for (_, n), p in ((ia, packed_a), (ib, packed_b)))
    both_a, both_b = np.isin(ia[0], ib[0]), np.isin(ib[0], ia[0])
    n_a, n_b, n_shared = len(a), len(b), int(both_a.sum())
    sum_a, sum_b, sum_min = int(a.sum()), int(b.sum()), int(np.minimum(a[both_a], b[both_b]).sum())
    return {"n_a": n_a, "n_b": n_b, "n_shared": n_shared, "sum_a": sum_a, "sum_b": sum_b, "sum_min": sum_min,
            "jaccard": n_shared / (n_a + n_b - n_shared) if n_a + n_b - n_shared else 0.0,
            "containment_a": n_shared / n_a if n_a else 0.0, "containment_b": n_shared / n_b if n_b else 0.0,
            "bray_curtis": 1.0 - 2.0 * sum_min / (sum_a + sum_b) if sum_a + sum_b else 0.0}


def _check_compare(A, B, ia, ib):
    before = A.data.clone(), B.data.clone()
    got = A.compare(B)
    want = _compared(ia, ib, A.kind in PACKED, B.kind in PACKED)
    assert list(got) == list(want)
    assert all(type(got[f]) is int for f in ("n_a", "n_b", "n_shared", "sum_a", "sum_b", "sum_min"))
    assert all(type(got[f]) is float for f in ("jaccard", "containment_a", "containment_b", "bray_curtis"))
    assert got == want
    assert torch.equal(A.data, before[0]) and torch.equal(B.data, before[1])
    return got


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_compare_same_kind(case):
    A, B, ia, ib = merge._pair(case)
    got = _check_compare(A, B, ia, ib)
    assert 0 < got["n_shared"] < min(got["n_a"], got["n_b"]) and 0.0 < got["jaccard"] < 1.0 and 0.0 < got["bray_curtis"] < 1.0
    same = _check_compare(A, A, ia, ia)
    assert same["jaccard"] == 1.0 and same["containment_a"] == 1.0 and same["bray_curtis"] == 0.0


@pytest.mark.parametrize("src,dst,k", CROSS, ids=[f"{s}-x-{d}-k{k}" for s, d, k in CROSS])
def test_compare_cross_kind(src, dst, k):
    A, B, ia, ib = _cross_pair(src, dst, k)
    _check_compare(A, B, ia, ib)
    _check_compare(B, A, ib, ia)


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: c[0])
def test_compare_disjoint_and_empty(case):
    A, Cc, ia, ic = _disjoint_pair(case)
    got = _check_compare(A, Cc, ia, ic)
    assert got["n_shared"] == 0 and got["jaccard"] == 0.0 and got["bray_curtis"] == 1.0
    none = (np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    empty = merge._fresh(*case)
    got = _check_compare(A, empty, ia, none)
    assert got["n_b"] == 0 and got["containment_b"] == 0.0
    got = _check_compare(empty, merge._fresh(*case), none, none)
    assert all(v == 0 for v in got.values())


# 9 ---- the tool
def _tool(*argv):
    try:
        return cli.main_kmer_table([str(a) for a in argv])
    except SystemExit as e:
        return e.code


def _g(name):
    return os.path.join(GOLDEN, name)


def _reloaded(path, k):
    codes, counts = oracle.Table.from_dump(str(path), k).items()
    return np.asarray(codes, dtype=np.uint64), np.asarray(counts).astype(np.int64)


def test_kmer_table_combine_compare_and_dump_upper(tmp_path, monkeypatch, capsys):
    monkeypatch.delenv("PANGAEA_LOWERCASE_IS_BASE", raising=False)
    out = tmp_path / "out.dump"
    k = 15
    # two dumps, written by the oracle from the two overlapping texts
    a, b, ia, ib = merge._texts(k, 60_000)
    da, db = tmp_path / "a.dump", tmp_path / "b.dump"
    oracle.Table(k, threads=4).count(a).dump(str(da))
    oracle.Table(k, threads=4).count(b).dump(str(db))
    for op, window, flags in (("min", (1, None), ()), ("max", (1, None), ()), ("diff", (1, None), ()), ("left", (2, None), ("-L", 2)),
                              ("only", (1, 1), ("-U", 1)), ("max", (2, 3), ("-L", 2, "-U", 3))):
        want = _expected(ia, ib, op, True, True, True, *window)
        assert 0 < len(want[0]) and (window == (1, None) and op == "max" or len(want[0]) < len(np.union1d(ia[0], ib[0])))
        assert _tool("combine", "--op", op, "-k", k, "-ga", da, "-gb", db, *flags, "-o", out) == 0
        got = _reloaded(out, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), op
    # a dump and reads: the dump holds half of the reads' text (a quarter of it twice) and a text of its own; the reads are counted
    # with jellyfish's rule (lower-case bases count)
    seq = oracle.Reads(_g("soft.fq")).all_seq()
    mixed = oracle.Table(k).count(seq[:len(seq) // 2], lowercase_is_base=True).count(seq[:len(seq) // 4], lowercase_is_base=True).count(a[:3_000])
    dm = tmp_path / "mixed.dump"
    mixed.dump(str(dm))
    im, counted = mixed.items(), oracle.Table(k).count(seq, lowercase_is_base=True).items()
    for op in OPS:
        want = _expected(im, counted, op, True, True, True)
        assert 0 < len(want[0]) and (op == "max" or len(want[0]) < len(np.union1d(im[0], counted[0])))
        assert _tool("combine", "--op", op, "-k", k, "-ga", dm, "-ib", _g("soft.fq"), "-o", out) == 0
        got = _reloaded(out, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), op
    # dump -U: the subset; without -U the bytes write_dump gives
    want = _expected(ia, None, "keep", True, lower=2, upper=4)
    assert 0 < len(want[0]) < (ia[1] >= 2).sum()
    assert _tool("dump", "-k", k, "-g", da, "-L", 2, "-U", 4, "-o", out) == 0
    got = _reloaded(out, k)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # (two loads of one dump may place colliding keys in another order: the bytes are compared on ONE loaded table, which the tool
    # is handed in place of its own load; the lines of its own load are compared as a set)
    plain = tmp_path / "plain.dump"
    loaded = kmer.KmerTable.from_dump(str(da), k, torch.device(DEV))
    loaded.write_dump(str(plain), 2)
    assert _tool("dump", "-k", k, "-g", da, "-L", 2, "-o", out) == 0
    assert sorted(open(out, "rb").read().splitlines()) == sorted(open(plain, "rb").read().splitlines()) and os.path.getsize(out) > 0
    with monkeypatch.context() as m:
        m.setattr(cli, "_table_for", lambda args: loaded)
        assert _tool("dump", "-k", k, "-g", da, "-L", 2, "-o", out) == 0
    assert open(out, "rb").read() == open(plain, "rb").read()
    # compare: the JSON of compare()
    capsys.readouterr()
    assert _tool("compare", "-k", k, "-ga", dm, "-ib", _g("soft.fq")) == 0
    printed = capsys.readouterr().out
    assert printed.endswith("\n") and printed.count("\n") == 1
    want = _compared(im, counted, True, True)
    assert json.loads(printed) == want and 0 < want["n_shared"] < min(want["n_a"], want["n_b"])
