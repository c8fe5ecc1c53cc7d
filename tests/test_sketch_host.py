"""The reference of the HyperLogLog sizing sketch (tests/_sketch_ref.py) checked by itself, ``kmer.sketch_estimate`` against it, and
the argument checks of ``pg_kmer_distinct_sketch`` -- all without a GPU.

What tests/test_sketch_gpu.py compares the kernel's registers with is pinned here first: the numpy path over the text against the
oracle's table at every k, the hash inversion behind the extreme ranks, the estimator against the truth across its range (the one
statistical statement, about the reference alone), and -- ``test_inputs_discriminate`` -- that each deliberate mistake of
``_sketch_ref.FAULTS`` changes the registers of the input the GPU file runs for it."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle
from pangaea_amd import _lib, kmer

from . import _corpus
from . import _sketch_ref as ref

OK, EINVAL = 0, -1
KS = list(range(1, 32))
SHIFTS = (0, 1, 31)
SEEDS = (0, 1, 2)
CARDINALITIES = (100, 1_000, 4_096, 8_000, 10_240, 12_000, 15_000, 20_000, 30_000, 50_000, 200_000, 1_000_000)
SWEEP_KS = (11, 21, 31)
BOUND = 4 * 1.04 / np.sqrt(ref.M)                   # 4 standard errors of HyperLogLog at m = 4096: 6.5 %
MARGIN = 0.05                                       # what dist.py adds to the estimate of the union before it sizes the table


# ------------------------------------------------------------------ the reference against itself


@pytest.mark.parametrize("k", KS)
def test_numpy_path_equals_the_oracle_table(k):
    """``registers_of_text`` (numpy over the text) == ``registers_of_codes`` of the oracle's keys, on the edge-case corpus at three
    alignments against the word grid, under both rules for lower-case bases"""
    reads = _corpus.corpus(k)
    for shift in SHIFTS:
        text = _corpus.stream_of(reads, shift).text
        for lc in (False, True):
            codes = oracle.Table(k, threads=2).count(text, lc).items()[0]
            assert len(codes) and np.array_equal(ref.canonical_codes(text, k, lowercase_is_base=lc), codes)
            assert np.array_equal(ref.registers_of_text(text, k, lowercase_is_base=lc), ref.registers_of_codes(codes))
        assert np.array_equal(ref.canonical_codes(text, k, plane=_packed_valid(text)), ref.canonical_codes(text, k))


def _packed_valid(text: bytes) -> np.ndarray:
    ok = np.isin(np.frombuffer(text, dtype=np.uint8), list(b"ACGT"))
    ok = np.concatenate([ok, np.zeros(-len(ok) % ref.WORD, dtype=bool)])
    return (ok.reshape(-1, ref.WORD).astype(np.uint32) << np.arange(ref.WORD, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)


def test_a_plane_is_the_text_with_n():
    """``plane=``: the k-mers under a thinned plane are those of the text with the cleared characters replaced by N; and a range of
    characters owns the k-mers that END in it"""
    text = ref.range_text()
    plane = ref.thinned(_packed_valid(text))
    kept = ref.plane_bits(plane, len(text))
    as_n = np.where(kept, np.frombuffer(text, dtype=np.uint8), np.uint8(ord("N"))).tobytes()
    assert 0.015 < 1 - kept.sum() / (len(text) - text.count(b"N")) < 0.025
    for k in (21, 31):
        assert np.array_equal(ref.canonical_codes(text, k, plane), oracle.Table(k).count(as_n).items()[0])
        whole = ref.registers_of_text(text, k)
        for c in ref.RANGE_CUTS:
            head = ref.registers_of_text(text, k, 0, 32 * c)
            assert np.array_equal(head, ref.registers_of_codes(oracle.Table(k).count(text[:32 * c]).items()[0]))
            assert np.array_equal(ref.combine(head, ref.registers_of_text(text, k, 32 * c)), whole)


def test_hash_and_its_inverse():
    x = np.random.RandomState(0).randint(0, 1 << 62, size=10_000, dtype=np.int64).astype(np.uint64) * np.uint64(5)
    assert np.array_equal(ref.mix64_inverse(ref.mix64(x)), x) and np.array_equal(ref.mix64(ref.mix64_inverse(x)), x)
    assert int(ref.mix64(1)[0]) == _mix64_int(1) and int(ref.mix64(ref.XOR)[0]) == _mix64_int(ref.XOR)
    values = [0, 1, 2, 3, 1 << 11, (1 << 12) - 1, 1 << 63, (1 << 64) - 1, 1 << 32, (1 << 32) - 1]
    assert ref.clz64(values).tolist() == [64 - int(v).bit_length() for v in values]


def _mix64_int(x: int) -> int:
    """mix64 in Python integers"""
    for mul in (ref.MUL1, ref.MUL2):
        x ^= x >> 33
        x = (x * mul) & ((1 << 64) - 1)
    return x ^ (x >> 33)


@pytest.mark.parametrize("rank", [1, 2, 20, 33, 45, 52, 53])
def test_kmer_with(rank):
    """the 31-mer has exactly the rank asked for, in the register asked for or the first after it that has such a 31-mer; about
    one register in eight has one"""
    low = 0 if rank == ref.MAX_RANK else 1 << (52 - rank)
    codes = ref.mix64_inverse((np.arange(ref.M, dtype=np.uint64) << np.uint64(52)) | np.uint64(low)) ^ np.uint64(ref.XOR)
    has = [int(c) < 1 << 62 and int(c) <= int(ref.revcomp_codes(c, 31)[0]) for c in codes]
    assert abs(sum(has) - ref.M / 8) <= 4 * np.sqrt(ref.M * (1 / 8) * (7 / 8))        # (one in four is below 4^31, half of those canonical)
    for idx in (0, 1, 777, 2048, 4095):
        kmer_ = ref.kmer_with(idx, rank)
        want = next((idx + d) % ref.M for d in range(ref.M) if has[(idx + d) % ref.M])
        assert len(kmer_) == 31 and set(kmer_) <= set(b"ACGT")
        code = ref.code_of_kmer(kmer_)
        assert code == int(ref.canonical_of(code, 31)[0]) and ref.kmer_of_code(code, 31) == kmer_
        regs = ref.registers_of_codes([code])
        assert regs[want] == rank and np.count_nonzero(regs) == 1
        assert np.array_equal(ref.registers_of_text(kmer_, 31), regs) and np.array_equal(ref.registers_of_text(ref.revcomp(kmer_), 31), regs)
    assert ref.index_and_rank(ref.code_of_kmer(ref.RANK53))[1].tolist() == [53]


# ------------------------------------------------------------------ kmer.sketch_estimate == the restated estimator


def _few(n: int) -> np.ndarray:
    return ref.registers_of_codes(ref.distinct_canonical(21, n, seed=7))


def test_sketch_estimate_is_the_restated_estimator():
    one = np.zeros(ref.M, dtype=np.int64)
    one[1234] = 17
    cases = {"all zero": np.zeros(ref.M, dtype=np.int64), "one register": one,
             "no zero left, raw estimate below 2.5 m": np.ones(ref.M, dtype=np.int64),
             "no zero left, one high register": np.where(np.arange(ref.M) == 9, 53, 1),
             "all at 53": np.full(ref.M, 53, dtype=np.int64)}
    cases.update({f"{n} k-mers": _few(n) for n in range(1, 11)})
    cases.update({f"{n} k-mers": ref.registers_of_codes(ref.distinct_canonical(31, n, seed=3)) for n in (4_096, 10_240, 12_000, 200_000)})
    for name, regs in cases.items():
        got = kmer.sketch_estimate(torch.from_numpy(regs.astype(np.int32)))
        assert isinstance(got, int) and got == ref.estimate(regs), name
    assert ref.estimate(cases["all zero"]) == 0 and ref.estimate(one) == 1
    raw = 0.7213 / (1 + 1.079 / ref.M) * ref.M * ref.M / (ref.M / 2)
    assert raw <= 2.5 * ref.M and ref.estimate(np.ones(ref.M, dtype=np.int64)) == int(raw)          # (the `and zeros` branch: no log of m / 0)
    assert ref.estimate(cases["all at 53"]) == int(0.7213 / (1 + 1.079 / ref.M) * ref.M * 2 ** 53)
    for n in range(1, 11):                                                                         # exact while linear counting holds
        assert np.count_nonzero(cases[f"{n} k-mers"]) == n and ref.estimate(cases[f"{n} k-mers"]) == n


# ------------------------------------------------------------------ the estimator against the truth


@functools.lru_cache(maxsize=None)
def _sweep() -> dict:
    """{(k, seed, n): estimate} -- every cardinality is a prefix of one seeded draw of distinct canonical codes"""
    out = {}
    for k in SWEEP_KS:
        sizes = [n for n in CARDINALITIES if k > 11 or n <= 200_000]
        for seed in SEEDS:
            idx, rank = ref.index_and_rank(ref.distinct_canonical(k, sizes[-1], seed))
            regs = np.zeros(ref.M, dtype=np.int64)
            done = 0
            for n in sizes:
                np.maximum.at(regs, idx[done:n], rank[done:n])
                done = n
                out[k, seed, n] = ref.estimate(regs)
    return out


def sweep_table() -> str:
    """the docstring table of ``test_estimator_against_the_truth``"""
    got = _sweep()
    lines = ["           n  " + "  ".join(f"k={k} s={s}" for k in SWEEP_KS for s in SEEDS)]
    for n in CARDINALITIES:
        cells = [f"{100 * (got[k, s, n] - n) / n:+7.2f}" if (k, s, n) in got else "       " for k in SWEEP_KS for s in SEEDS]
        lines.append(f"    {n:>8}  " + "   ".join(cells))
    return "\n".join(lines)


def test_estimator_against_the_truth():
    """Relative error of ``estimate`` in percent, for n distinct canonical codes of ``distinct_canonical(k, n, seed)``
    (``sweep_table()`` prints this):

           n  k=11 s=0  k=11 s=1  k=11 s=2  k=21 s=0  k=21 s=1  k=21 s=2  k=31 s=0  k=31 s=1  k=31 s=2
         100    +0.00     +0.00     +0.00     +1.00     -1.00     +1.00     -1.00     +0.00     +0.00
        1000    +0.70     -0.50     -0.30     -3.80     -0.10     -0.60     +0.70     -0.10     -0.10
        4096    +0.17     -1.46     -1.22     -0.76     +0.51     -0.76     +1.12     +0.05     -1.07
        8000    +1.06     -2.67     +0.16     +0.70     +0.96     -0.45     +1.06     +1.51     +0.79
       10240    +2.80     +2.88     +4.02     +0.95     +3.47     +3.68     +2.29     +4.44     +0.41
       12000    +1.16     +2.80     +1.60     -0.50     +1.54     +1.74     +0.99     +2.37     -0.40
       15000    +1.13     +0.62     +0.72     -1.66     +0.25     -0.45     +0.40     +1.14     -0.48
       20000    -0.26     +0.48     -0.33     +0.13     +0.98     -1.08     -0.65     -0.57     -1.31
       30000    +1.29     +0.08     -0.11     -1.83     +2.76     -2.08     -0.43     -0.62     -3.19
       50000    -0.21     -2.14     -2.84     -0.35     +1.71     -0.28     +1.36     +0.35     +0.09
      200000    -0.87     +0.54     -0.74     -1.60     -0.51     +0.75     -0.86     -0.90     -0.31
     1000000                                  -1.35     -1.09     -1.83     -0.32     +0.23     +1.36

    (worst: +4.44 % at n = 10 240, -3.80 % at n = 1 000; 105 draws.)

    Every draw lies within 4 standard errors of HyperLogLog at m = 4096 (4 x 1.04 / sqrt(4096) = 6.5 %); the upward bias just
    above the switch of the estimator's form (n = 10 240 = 2.5 m) shows.  And no draw underestimates by more than 5 %: the
    margin ``dist.py`` adds to the estimate of the union before it sizes the common table -- with a larger underestimate the
    table would hold fewer slots than k-mers at load 1."""
    got = _sweep()
    assert len(got) == len(SEEDS) * (3 * len(CARDINALITIES) - 1) and abs(BOUND - 0.065) < 1e-12
    for (k, seed, n), est in got.items():
        error = (est - n) / n
        assert abs(error) <= BOUND, (k, seed, n, error)
        assert error >= -MARGIN, (k, seed, n, error)


# ------------------------------------------------------------------ the inputs of the GPU file discriminate


def _differs(a, b) -> bool:
    return not np.array_equal(a, b)


def test_inputs_discriminate():
    """every fault of ``_sketch_ref.FAULTS``, switched into the REFERENCE, changes the registers of the input that
    tests/test_sketch_gpu.py runs for it: a kernel with that fault fails there.  No faulty kernel runs anywhere."""
    seen = set()

    def fault(name):
        seen.add(name)
        return name

    text, n = ref.range_text(), ref.RANGE_WORDS * ref.WORD
    for k in (21, 31):
        true = ref.registers_of_text(text, k)
        # (a) random one-strand text, and a run of T (canonical: the all-A k-mer)
        assert _differs(ref.registers_of_text(text, k, fault=fault("forward")), true)
        assert _differs(ref.registers_of_text(ref.repeat_text(b"T"), k, fault="forward"), ref.registers_of_text(ref.repeat_text(b"T"), k))
        # (b), (c) the word ranges: at every cut some k-mer straddles; the tail behind the last cut and the head before the first
        # hold so few k-mers that the straddling ones must show
        ends = ref.kmers_of_text(text, k)[0]
        for c in ref.RANGE_CUTS:
            assert ((ends >= 32 * c) & (ends - k + 1 < 32 * c)).any(), c
        dropped = [c for c in ref.RANGE_CUTS
                   if _differs(ref.registers_of_text(text, k, 32 * c, n, fault=fault("drop-straddlers")), ref.registers_of_text(text, k, 32 * c, n))]
        by_start = [c for c in ref.RANGE_CUTS
                    if _differs(ref.registers_of_text(text, k, 0, 32 * c, fault=fault("own-by-start")), ref.registers_of_text(text, k, 0, 32 * c))]
        assert 4095 in dropped and 1 in by_start, (dropped, by_start)
        # (j) any k above 16
        assert _differs(ref.registers_of_text(text, k, fault=fault("code32")), true)
        # (f), (g) anything
        assert _differs(ref.registers_of_text(text, k, fault=fault("low-index")), true)
        assert _differs(ref.registers_of_text(text, k, fault=fault("rank-minus-one")), true)
    # (d) the corpus: reads of k - 1 characters, an N inside a read
    for k in (11, 21, 31):
        laid = _corpus.stream_of(_corpus.corpus(k), 1)
        assert _differs(ref.registers_of_text(laid.text, k, fault=fault("short-run")), ref.registers_of_text(laid.text, k))
    # (e) the all-A k-mer: code 0, which mix64 maps to 0
    for k in (1, 21, 31):
        one = ref.registers_of_text(ref.repeat_text(b"A"), k)
        assert np.count_nonzero(one) == 1
        assert _differs(ref.registers_of_text(ref.repeat_text(b"A"), k, fault=fault("no-xor")), one)
        assert _differs(ref.registers_of_text(ref.repeat_text(b"A"), k, fault="rank-minus-one"), one)
    # (h), (i) the 31-mers of rank 53
    for shift in (0, 17):
        extreme = ref.registers_of_text(ref.extreme_text(shift), 31)
        assert sorted(extreme[extreme > 0].tolist()) == sorted(ref.EXTREME_RANKS + (53,)) and extreme.max() == ref.MAX_RANK
        high = ref.registers_of_text(ref.extreme_text(shift), 31, fault=fault("no-sentinel"))
        assert _differs(high, extreme) and high.max() == 65
        low = ref.registers_of_text(ref.extreme_text(shift), 31, fault=fault("sentinel-high"))
        assert _differs(low, extreme) and low.max() == 52
    # (k) 32 workgroups' registers, every one contended
    ends, codes = ref.kmers_of_text(ref.contended_text(), 21)
    true = ref.registers_of_codes(codes)
    assert np.array_equal(true, ref.registers_of_codes(oracle.Table(21, threads=4).count(ref.contended_text()).items()[0])) and true.min() > 0
    block = ends // (ref.BLOCK_WORDS * ref.WORD)
    parts = [ref.registers_of_codes(codes[block == b]) for b in range(ref.CONTENDED_WORDS // ref.BLOCK_WORDS)]
    assert len(parts) == 32 and np.array_equal(functools.reduce(ref.combine, parts), true)
    assert _differs(functools.reduce(lambda a, b: ref.combine(a, b, fault=fault("overwrite")), parts), true)
    assert seen == set(ref.FAULTS)


def test_trip_islands_lie_where_the_grid_stride_loop_can_lose_them():
    """the islands of ``trip_text``: in the first and the last word, and across the word boundaries at which one workgroup's
    share ends, the first trip of the grid ends, and the second trip's first share ends"""
    starts = ref.island_starts()
    assert ref.TRIP_WORDS > 1024 * ref.BLOCK_WORDS and starts[0] == 0 and starts[-1] + ref.ISLAND == ref.TRIP_WORDS * ref.WORD
    for at, w in zip(starts[1:-1], (1024, 1 << 20, (1 << 20) + 1024)):
        assert at < w * ref.WORD - 31 and at + ref.ISLAND > w * ref.WORD + 31
    assert all(b - a > ref.ISLAND for a, b in zip(starts, starts[1:]))
    codes = np.unique(np.concatenate([ref.canonical_codes(island, 31) for island in ref.trip_islands()]))
    assert len(codes) == len(starts) * (ref.ISLAND - 30)


# ------------------------------------------------------------------ the C entry refuses before it touches the device


def test_entry_refuses_bad_arguments():
    L = _lib.load()
    codes = np.zeros(4, dtype=np.uint64)
    valid = np.zeros(4, dtype=np.uint32)
    regs = np.zeros(ref.M, dtype=np.uint32)
    c, v, r = codes.ctypes.data, valid.ctypes.data, regs.ctypes.data

    def call(codes_=c, valid_=v, regs_=r, begin=0, end=4, k=21):
        return L.pg_kmer_distinct_sketch(codes_, valid_, begin, end, k, regs_, None)

    assert call(codes_=None) == EINVAL and call(valid_=None) == EINVAL and call(regs_=None) == EINVAL
    assert L.pg_last_error().decode() == "pg_kmer_distinct_sketch: null argument"
    assert call(k=0) == EINVAL and call(k=32) == EINVAL and call(k=-1) == EINVAL
    assert call(begin=-1) == EINVAL and call(begin=3, end=2) == EINVAL and call(begin=-2, end=-2) == EINVAL
    assert L.pg_last_error().decode() == "pg_kmer_distinct_sketch: bad word range"
    for at in (0, 2, 4):                       # an empty range with host pointers: nothing is read, nothing is launched
        assert call(begin=at, end=at, k=1) == OK and call(begin=at, end=at, k=31) == OK
    assert not regs.any()
