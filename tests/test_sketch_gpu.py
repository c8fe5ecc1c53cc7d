"""``distinct_sketch_kernel`` (pangaea_amd/csrc/kernels.hip), the kernel every table without a size hint is sized from, register
for register against tests/_sketch_ref.py: ``np.array_equal`` on the 4096 registers, no tolerance anywhere.

The expected registers come from the oracle's table (the registers depend on the SET of canonical codes alone) or from the numpy
path of the reference, which tests/test_sketch_host.py checks against the oracle; that file also shows that each mistake of
``_sketch_ref.FAULTS`` would change the registers of the input used for it here.

  test_every_k_on_the_corpus            load_word / runs_of / Roller as the kernel uses them, at every k and word alignment
  test_word_ranges                      word_begin / word_end: a k-mer belongs to the word it ENDS in; max of parts = whole
  test_one_register                     a whole workgroup's atomicMax on one LDS register
  test_many_workgroups                  LDS registers -> global registers with every register contended
  test_second_trip_of_the_grid          the grid-stride loop, and the ends of every workgroup's share
  test_extreme_ranks                    the sentinel bit: rank 53 and never more
  test_plane_*                          ``plane=``: the plane given is the one used
  test_accumulates_*                    registers that are not zero; several calls into one array
  test_side_stream                      the launch goes to the current stream
  test_shards_combine_by_max            the identity dist.py's all-reduce(MAX) rests on
  test_estimate_end_to_end              ``kmer.estimate_distinct`` = the restated estimator of the expected registers"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from pangaea_amd import _lib, kmer
from pangaea_amd.reads import ReadStream

from . import _corpus
from . import _sketch_ref as ref
from .conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = list(range(1, 32))
SHIFTS = (0, 1, 31)


def _regs(t: torch.Tensor) -> np.ndarray:
    assert t.dtype == torch.int32 and t.shape == (ref.M,)
    return t.cpu().numpy().astype(np.int64)


def _stream(text: bytes) -> ReadStream:
    s = ReadStream.from_runs([("r", text)], device=DEV)
    assert s.n_chars == len(text) and s.n_words * ref.WORD >= len(text)
    return s


def _of_table(text: bytes, k: int, lowercase_is_base: bool = False) -> np.ndarray:
    return ref.registers_of_codes(oracle.Table(k, threads=4).count(text, lowercase_is_base).items()[0])


@functools.lru_cache(maxsize=None)
def _range_case():
    """the text of the word ranges, its stream, and its registers at k = 21 and 31; shared, never written to"""
    text = ref.range_text()
    return text, _stream(text), {k: _of_table(text, k) for k in (21, 31)}


# ------------------------------------------------------------------ every k, every alignment


@pytest.mark.parametrize("k", KS)
def test_every_k_on_the_corpus(k):
    """reads shorter than k, an N and a lower-case stretch at every offset of a word, periodic reads, palindromes, every read's
    reverse complement, at three alignments against the word grid; lower-case bases as no bases and as bases"""
    reads = _corpus.corpus(k)
    for shift in SHIFTS:
        laid = _corpus.stream_of(reads, shift)
        s = ReadStream.from_runs(laid.runs, device=DEV)
        assert s.valid_lower is not None and s.n_words >= laid.n_words > 4096
        strict, lenient = _of_table(laid.text, k), _of_table(laid.text, k, True)
        assert np.array_equal(_regs(kmer.distinct_sketch(s, k)), strict), shift
        assert np.array_equal(_regs(kmer.distinct_sketch(s, k, lowercase_is_base=True)), lenient), shift


# ------------------------------------------------------------------ word ranges


@pytest.mark.parametrize("k", [21, 31])
def test_word_ranges(k):
    """[0, c) holds the k-mers that end before character 32 c, [c, n) the rest -- those that straddle the cut included --, their
    maximum is the whole, and an empty range leaves the registers zero"""
    text, s, whole = _range_case()
    n = s.n_words
    assert n >= ref.RANGE_WORDS
    got_whole = kmer.distinct_sketch(s, k, 0, n)
    assert np.array_equal(_regs(got_whole), whole[k])
    for c in ref.RANGE_CUTS:
        assert 0 < c < n
        head, tail = kmer.distinct_sketch(s, k, 0, c), kmer.distinct_sketch(s, k, c, n)
        assert np.array_equal(_regs(head), ref.registers_of_text(text, k, 0, 32 * c)), c
        assert np.array_equal(_regs(tail), ref.registers_of_text(text, k, 32 * c)), c
        assert torch.equal(torch.maximum(head, tail), got_whole), c
        assert not kmer.distinct_sketch(s, k, c, c).any(), c
    assert not kmer.distinct_sketch(s, k, 0, 0).any() and not kmer.distinct_sketch(s, k, n, n).any()


# ------------------------------------------------------------------ contention


@pytest.mark.parametrize("unit", [b"A", b"T", b"AC", b"ACG"])
def test_one_register(unit):
    """2048 words of one repeated unit: every lane of two workgroups raises the same one or two LDS registers"""
    text = ref.repeat_text(unit)
    s = _stream(text)
    for k in (1, 16, 21, 31):
        want = _of_table(text, k)
        distinct = len(oracle.Table(k).count(text))
        assert distinct == {b"A": 1, b"T": 1}.get(unit, distinct) <= 3
        got = _regs(kmer.distinct_sketch(s, k))
        assert np.array_equal(got, want) and 1 <= np.count_nonzero(got) <= distinct, k


def test_many_workgroups():
    """2^15 words of random bases at k = 21: a million k-mers in 32 workgroups, every global register raised by most of them"""
    text = ref.contended_text()
    s = _stream(text)
    want = _of_table(text, 21)
    assert want.min() > 0 and s.n_words >= 32 * ref.BLOCK_WORDS
    assert np.array_equal(_regs(kmer.distinct_sketch(s, 21)), want)


def test_second_trip_of_the_grid():
    """more than 1024 x 1024 words, so that the first workgroups take a second trip of the grid-stride loop: N everywhere but for
    islands of random bases in the first word, across the end of the first workgroup's share, across the end of the first trip,
    across the end of the first share of the second trip, and in the last word.  k = 31."""
    s = _stream(ref.trip_text().tobytes())
    assert s.n_words >= ref.TRIP_WORDS > 1024 * ref.BLOCK_WORDS
    codes = np.unique(np.concatenate([ref.canonical_codes(island, 31) for island in ref.trip_islands()]))
    got = _regs(kmer.distinct_sketch(s, 31))
    assert np.array_equal(got, ref.registers_of_codes(codes))
    per_island = [ref.registers_of_text(island, 31) for island in ref.trip_islands()]
    assert all((got >= r).all() and r.any() for r in per_island)


# ------------------------------------------------------------------ the ends of the rank's range


@pytest.mark.parametrize("shift", [0, 17])
def test_extreme_ranks(shift):
    """31-mers whose hashes have the ranks 1, 2, 33, 52 and 53 (tests/_sketch_ref.py: kmer_with), two of them also as their reverse
    complements; at shift 17 every one of them straddles a word.  53 is reached and nothing beyond."""
    text = ref.extreme_text(shift)
    got = _regs(kmer.distinct_sketch(_stream(text), 31))
    assert np.array_equal(got, ref.registers_of_text(text, 31)) and np.array_equal(got, _of_table(text, 31))
    assert got.max() == ref.MAX_RANK == 53 and sorted(got[got > 0].tolist()) == [1, 2, 33, 52, 53, 53]


# ------------------------------------------------------------------ plane=


@pytest.mark.parametrize("k", [21, 31])
def test_plane_of_the_callers_own(k):
    """``stream.valid`` with a seeded 2 % of its set bits cleared == the text with those characters replaced by N"""
    text, s, whole = _range_case()
    words = ref.thinned(s.valid.cpu().numpy())
    kept = ref.plane_bits(words, len(text))
    as_n = np.where(kept, np.frombuffer(text, dtype=np.uint8), np.uint8(ord("N"))).tobytes()
    plane = torch.from_numpy(words.view(np.int32)).to(DEV)
    want = _of_table(as_n, k)
    assert not np.array_equal(want, whole[k])
    assert np.array_equal(_regs(kmer.distinct_sketch(s, k, plane=plane)), want)
    assert np.array_equal(_regs(kmer.distinct_sketch(s, k, plane=plane, lowercase_is_base=True)), want)       # (the plane given wins)


def _check_planes(s: ReadStream, text: bytes, ks) -> int:
    """the three planes the masked N-rank form sketches with, each against the k-mers of the text under that plane; how many of
    the three differ"""
    planes = [s.table_valid(True), s.table_valid(False), s.union_valid(True)]
    for k in ks:
        for plane in planes:
            want = ref.registers_of_codes(ref.canonical_codes(text, k, plane.cpu().numpy()))
            assert want.any() and np.array_equal(_regs(kmer.distinct_sketch(s, k, plane=plane)), want), k
        assert torch.equal(kmer.distinct_sketch(s, k, lowercase_is_base=True), kmer.distinct_sketch(s, k, plane=planes[0]))
        assert torch.equal(kmer.distinct_sketch(s, k), kmer.distinct_sketch(s, k, plane=planes[1]))
    return len({p.cpu().numpy().tobytes() for p in planes})


def test_plane_of_quality_masked_pairs():
    """the paired golden FASTQ files, which carry a quality plane: the table's plane leaves the low-quality bases out, the union
    plane (what a masked count half holds in its local slots) does not"""
    s = ReadStream.from_fastq(os.path.join(GOLDEN, "pairq_R1.fq"), os.path.join(GOLDEN, "pairq_R2.fq"), device=DEV)
    assert s.valid_lowq is not None
    assert _check_planes(s, s.decode(plane=s.lenient_valid()), (15, 21)) == 2


def test_plane_of_the_masked_corpus():
    """quality marks AND lower-case stretches (tests/_corpus.py: masked_corpus): three planes that all differ"""
    k = 21
    laid = _corpus.masked_stream_of(_corpus.masked_corpus(k), 1, k)
    s = _corpus.host_stream(laid).to(DEV)
    assert s.valid_lowq is not None and s.valid_lower is not None
    assert _check_planes(s, laid.text, (k,)) == 3
    want = {lc: _of_table(laid.table_text(lc), k) for lc in (False, True)}
    assert not np.array_equal(want[False], want[True])            # (in the plain corpus every soft-masked k-mer is elsewhere in upper case)
    for lc in (False, True):
        assert np.array_equal(_regs(kmer.distinct_sketch(s, k, lowercase_is_base=lc)), want[lc])


# ------------------------------------------------------------------ accumulation, the stream


def _raw_sketch(s: ReadStream, k: int, begin: int, end: int, regs: torch.Tensor) -> None:
    assert 0 <= begin <= end <= s.n_words and regs.dtype == torch.int32 and regs.numel() == ref.M and regs.is_cuda
    stream = torch.cuda.current_stream(regs.device).cuda_stream
    _lib.check(_lib.load().pg_kmer_distinct_sketch(s.codes.data_ptr(), s.valid.data_ptr(), begin, end, k, regs.data_ptr(), stream))


@pytest.mark.parametrize("k", [21, 31])
def test_accumulates_into_the_registers_it_is_given(k):
    """two calls over two ranges into ONE array zeroed once == the sketch of the whole; and registers that hold something are
    raised, never lowered"""
    text, s, whole = _range_case()
    for c in (1, 1025, 4095):
        regs = torch.zeros(ref.M, dtype=torch.int32, device=DEV)
        _raw_sketch(s, k, 0, c, regs)
        _raw_sketch(s, k, c, s.n_words, regs)
        assert np.array_equal(_regs(regs), whole[k]), c
    held = torch.from_numpy((np.arange(ref.M) % 9).astype(np.int32)).to(DEV)
    before = _regs(held)
    _raw_sketch(s, k, 0, s.n_words, held)
    assert np.array_equal(_regs(held), np.maximum(before, whole[k])) and (before > whole[k]).any() and (before < whole[k]).any()


def test_side_stream():
    """the way bench.py and feature.py run it: under ``torch.cuda.stream(side)`` the launch goes to that stream"""
    text, s, whole = _range_case()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = [kmer.distinct_sketch(s, k) for k in (21, 31)]
    side.synchronize()
    for k, regs in zip((21, 31), got):
        assert np.array_equal(_regs(regs), whole[k]) and torch.equal(regs, kmer.distinct_sketch(s, k))


# ------------------------------------------------------------------ shards


@pytest.mark.parametrize("k", [15, 21, 31])
def test_shards_combine_by_max(k):
    """three streams from disjoint thirds of a read set: the maximum of their sketches is the sketch of the union of their
    three tables"""
    rng = np.random.RandomState(3)
    reads = [ref.random_bases(rng, 100 + i % 101).tobytes() for i in range(600)]
    for i in range(0, 200, 7):                                     # (some k-mers in two shards, on the other strand)
        reads[i] = _corpus.revcomp(reads[i + 200])
    third = len(reads) // 3
    sketches, tables = [], []
    for part in range(3):
        runs = [(f"r{i}", r + b"N") for i, r in enumerate(reads[part * third:(part + 1) * third])]
        sketches.append(kmer.distinct_sketch(ReadStream.from_runs(runs, device=DEV), k))
        tables.append(oracle.Table(k).count(b"".join(t for _, t in runs)).items()[0])
        assert np.array_equal(_regs(sketches[-1]), ref.registers_of_codes(tables[-1]))
    union = functools.reduce(np.union1d, tables)
    assert len(union) > max(len(t) for t in tables)
    combined = torch.maximum(torch.maximum(sketches[0], sketches[1]), sketches[2])
    assert np.array_equal(_regs(combined), ref.registers_of_codes(union))
    assert kmer.sketch_estimate(combined) == ref.estimate(ref.registers_of_codes(union))


# ------------------------------------------------------------------ the estimate


def test_estimate_end_to_end():
    """``kmer.estimate_distinct`` == the restated estimator of the expected registers, as an integer"""
    text, s, whole = _range_case()
    for k in (21, 31):
        assert kmer.estimate_distinct(s, k) == ref.estimate(whole[k])
        assert kmer.estimate_distinct(s, k, 256, 1025) == ref.estimate(ref.registers_of_text(text, k, 32 * 256, 32 * 1025))
    contended = ref.contended_text()
    assert kmer.estimate_distinct(_stream(contended), 21) == ref.estimate(_of_table(contended, 21))
    laid = _corpus.stream_of(_corpus.corpus(11), 31)
    s11 = ReadStream.from_runs(laid.runs, device=DEV)
    for lc in (False, True):
        assert kmer.estimate_distinct(s11, 11, lowercase_is_base=lc) == ref.estimate(_of_table(laid.text, 11, lc))
