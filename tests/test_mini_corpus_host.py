"""The edge-case corpus of tests/_corpus.py and the oracle on it, at every k of the super-k-mer pipeline -- no GPU.

tests/test_mini_corpus_gpu.py compares the kernels with the oracle's table and rows of this corpus, and with themselves under a
reverse complement and a shift of the stream.  What those checks rest on is checked here: the corpus holds what it claims, its
layout puts k-mers across the chunk and round boundaries at every shift, and the ORACLE's table is the same for the reverse
complemented stream and for every shift (rows too)."""
import numpy as np
import pytest

from oracle import oracle

from . import _corpus

KS = list(range(13, 32))


def _same_items(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_revcomp_and_periodic_units():
    assert _corpus.revcomp(b"AACGtN") == b"NaCGTT" and _corpus.revcomp(b"") == b""
    rng = np.random.RandomState(3)
    for p in range(1, 13):
        u = _corpus._unit(rng, p)
        assert len(u) == p and all(u != u[:d] * (p // d) for d in range(1, p) if p % d == 0)


@pytest.mark.parametrize("k", KS)
def test_corpus_holds_what_it_claims(k):
    reads = _corpus.corpus(k)
    assert reads == _corpus.corpus(k) and reads != _corpus.corpus(k, seed=1)              # deterministic, seeded
    half = len(reads) // 2
    fwd = reads[:half]
    assert reads[half:] == [_corpus.revcomp(r) for r in fwd]                               # (f)
    n_a = 2 * k + 41
    assert [len(r) for r in fwd[:n_a]] == list(range(n_a))                                 # (a)
    b, c = fwd[n_a:n_a + 96], fwd[n_a + 96:n_a + 192]
    base = c[0].upper()
    assert len(base) == 96 and set(base) <= set(b"ACGT")
    for j in range(96):                                                                    # (b), (c)
        assert b[j] == base[:j] + b"N" + base[j + 1:]
        low = [i for i in range(96) if c[j][i:i + 1].islower()]
        assert c[j].upper() == base and low == list(range(j, min(96, j + 1 + j % 3)))
    d = fwd[n_a + 192:n_a + 204]
    for p, r in enumerate(d, start=1):                                                     # (d)
        assert len(r) == 150 + p and r == (r[:p] * 200)[:len(r)]
    assert d[0] == b"A" * 151 and d[1].startswith(b"ACAC") and d[2].startswith(b"ACGACG")
    e = fwd[n_a + 204:]
    assert len(e) == 36
    for h, r in zip(range(4, 40), e):                                                      # (e)
        x = r[_corpus.FLANK:_corpus.FLANK + h]
        assert len(r) == 2 * _corpus.FLANK + 2 * h and r[_corpus.FLANK + h:_corpus.FLANK + 2 * h] == _corpus.revcomp(x)
    assert 614 <= len(reads) <= 686


@pytest.mark.parametrize("k", KS)
def test_layout_and_oracle_invariants(k):
    reads = _corpus.corpus(k)
    laid = _corpus.stream_of(reads, 0, k)                                                  # (asserts the layout's own claims)
    n = len(reads)
    assert laid.reads[:n] == reads and laid.reads[n:2 * n] == reads[::-1] and sorted(laid.reads[2 * n:]) == sorted(reads)
    assert laid.reads[2 * n:] != reads and len(laid.names) == len(set(laid.names))
    # a row per read, two in the second copy (but for the reads of 0 and 1 characters and their reverse complements)
    assert np.array_equal(np.bincount(laid.read_of_row), [1] * n + [1 if len(r) < 2 else 2 for r in reads[::-1]] + [1] * n)
    assert len(laid.names) == 4 * n - 4
    rows = laid.rows()
    assert (rows.end > rows.start).all() and (rows.start[1:] == rows.end[:-1]).all() and rows.end[-1] == len(laid.text)
    table = oracle.Table(k, threads=2).count(laid.text)
    _corpus.check_against_oracle(laid, k, table)
    assert 0 < _corpus.n_reads_with_a_kmer(laid, k) < len(laid.reads)
    # the Python count of the records: one per k-mer under a cap of 1 (the abundance rows hold every k-mer of the strict plane
    # once: (10, 400) drops none), fewer under 2, fewest under the cap of this k; records of more than four k-mers need a cap above 4
    m, w, delay, cap = _corpus.mini_geometry(k)
    assert (w, delay) == (k - m + 1, 0) if k <= 21 else w + 2 * delay == k - 12 and 1 <= delay <= 5
    assert cap == {13: 3, 21: 9, 31: 2}.get(k, cap) and 2 <= cap <= 9
    n_kmers = int(laid.rows_by_oracle(lambda seq: oracle.abd_row(seq, k, table, 10, 400)).sum())
    by_cap = [_corpus.count_records(laid, k, c) for c in (1, 2, None)]
    assert by_cap[0] == (n_kmers, 0) and by_cap[1][1] == 0 and (by_cap[2][1] > 0) == (cap > 4)
    assert by_cap[0][0] > by_cap[1][0] >= by_cap[2][0] > _corpus.n_reads_with_a_kmer(laid, k)
    # lower-case bases are no bases for the oracle's table, and are bases under jellyfish's rule
    assert _same_items(table.items(), oracle.Table(k).count(laid.text.replace(b"a", b"N").replace(b"c", b"N").replace(b"g", b"N").replace(b"t", b"N")).items())
    lenient = oracle.Table(k).count(laid.text.upper()).items()
    assert np.array_equal(lenient[0], table.items()[0]) and int(lenient[1].sum()) > int(table.items()[1].sum())   # (counts only: (b) holds every k-mer of (c))
    # the reverse complemented stream: the same table
    rc = _corpus.stream_of([_corpus.revcomp(r) for r in reversed(reads)], 0, k)
    assert rc.text != laid.text and _same_items(oracle.Table(k, threads=2).count(rc.text).items(), table.items())
    # every shift against the word grid: the same table, the same rows
    want = laid.rows_by_oracle(lambda seq: oracle.abd_row(seq, k, table, 1, 64))
    assert (want >= 0).all() and np.array_equal(np.add.reduceat(want, np.flatnonzero(np.diff(laid.read_of_row, prepend=-1))),
                                                np.stack([oracle.abd_row(r, k, table, 1, 64) for r in laid.reads]))
    for j in range(1, 32):
        s = _corpus.stream_of(reads, j, k)
        assert s.text == b"N" * j + laid.text and s.runs[0] == ("", b"N" * j) and s.names == laid.names
        assert np.array_equal(s.start, laid.start + j) and np.array_equal(s.end, laid.end + j)
        assert _same_items(oracle.Table(k, threads=2).count(s.text).items(), table.items())
        if j in (1, 31):
            assert np.array_equal(s.rows_by_oracle(lambda seq: oracle.abd_row(seq, k, table, 1, 64)), want)
