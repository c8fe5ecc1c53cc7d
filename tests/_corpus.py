"""An edge-case read corpus for the super-k-mer kernels (pangaea_amd/csrc/mini.hip), built for one k from a seeded random base
sequence -- what ``synth.generate`` never produces: reads shorter than k, an N or a soft-masked base at every position of a
word, periodic reads that reach the record cap, palindromic M-mers and k-mers, and every read's reverse complement.

``corpus(k, seed)`` is the list of reads (bytes, no separator).  ``stream_of(reads, shift, k)`` lays it out three times (in order,
reversed, in a seeded permutation), every read followed by ``N`` and a run of its own -- and a row of its own, or two in the
second copy, whose row boundaries lie inside records --, behind ``shift`` N's that move the whole text against the 32-character
word grid.  ``check_against_oracle`` makes the assertions that need the oracle's table.
A plain module: the host test (tests/test_mini_corpus_host.py) checks it at every k, the GPU test (tests/test_mini_corpus_gpu.py)
runs the kernels on it."""
from dataclasses import dataclass

import numpy as np

WORD = 32                         # characters per stream word
ROUND_CHARS = 512 * WORD          # a round of the first scatter pass (mini.hip: ROUND_WORDS)
CHUNK_CHARS = 4096 * WORD         # a chunk of the first scatter pass (mini.hip: MINI_CHUNK_WORDS)
BASE_LEN = 96                     # the read that carries the N and the lower-case stretch: three words
FLANK = 30
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(read: bytes) -> bytes:
    return read.translate(_COMP)[::-1]


def _random(rng, n: int) -> bytes:
    return bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8)) if n else b""


def _unit(rng, period: int) -> bytes:
    """a string whose smallest period is ``period``: A, AC, ACG, then random ones"""
    if period <= 3:
        return b"ACG"[:period]
    while True:
        u = _random(rng, period)
        if not any(period % d == 0 and u == u[:d] * (period // d) for d in range(1, period)):
            return u


def corpus(k: int, seed: int = 0) -> list:
    rng = np.random.RandomState(1000 * seed + k)
    reads = [_random(rng, n) for n in range(2 * k + 41)]                                        # (a) every length 0 .. 2k + 40
    base = _random(rng, BASE_LEN)
    reads += [base[:j] + b"N" + base[j + 1:] for j in range(BASE_LEN)]                           # (b) an N at each offset
    reads += [base[:j] + base[j:j + 1 + j % 3].lower() + base[j + 1 + j % 3:] for j in range(BASE_LEN)]   # (c) 1-3 lower-case bases
    for p in range(1, 13):                                                                      # (d) periodic: they reach the cap
        u = _unit(rng, p)
        reads.append((u * (150 // p + 2))[:150 + p])
    for h in range(4, 40):                                                                      # (e) palindromic M-mers and k-mers
        x = _random(rng, h)
        reads.append(_random(rng, FLANK) + x + revcomp(x) + _random(rng, FLANK))
    assert all(len(r) == BASE_LEN for r in reads[2 * k + 41:2 * k + 41 + 2 * BASE_LEN])
    return reads + [revcomp(r) for r in reads]                                                  # (f)


@dataclass
class Laid:
    """a corpus laid out as a stream: ``runs`` for ``ReadStream.from_runs``, the text, and the rows -- one per read (its run,
    the separator included: an empty read is a row of one N), except in the second copy, where every read of two characters and
    more is cut into two rows, so that row boundaries lie inside records"""
    runs: list
    text: bytes
    names: list
    start: np.ndarray
    end: np.ndarray
    reads: list            # the reads in stream order
    read_of_row: np.ndarray
    read_start: np.ndarray # per row: where its read starts

    def rows_by_oracle(self, fn) -> np.ndarray:
        """``fn(text)`` (a vector per text: ``oracle.abd_row``, ``oracle.tnf_row``) for every row.  A k-mer belongs to the row that
        holds its LAST character (include/pangaea_feat.h: 'the row its k-mer ends in'; for rows that are whole runs, the
        reference's own rule): the second part of a cut read gets the read's k-mers less those that lie in the first part."""
        out = []
        for a0, a, b in zip(self.read_start, self.start, self.end):
            v = fn(self.text[a0:b])
            out.append(v - fn(self.text[a0:a]) if a > a0 else v)
        return np.stack(out)

    @property
    def n_words(self) -> int:
        return -(-len(self.text) // WORD)

    def rows(self):
        from pangaea_amd.reads import Rows
        first = len(self.runs) - len(self.reads)               # (the unnamed run of the shift comes first)
        return Rows(first + self.read_of_row.astype(np.int64), list(self.names), self.start.copy(), self.end.copy())


def _valid_prefix(text: bytes) -> np.ndarray:
    t = np.frombuffer(text, dtype=np.uint8)
    ok = (t == ord("A")) | (t == ord("C")) | (t == ord("G")) | (t == ord("T"))
    return np.concatenate([[0], np.cumsum(ok)])


def kmer_crosses(prefix: np.ndarray, at: int, k: int) -> bool:
    """does a k-mer of upper-case bases begin before character ``at`` and end at or after it?"""
    lo, hi = max(0, at - k + 1), min(at - 1, len(prefix) - 1 - k)
    if hi < lo:
        return False
    i = np.arange(lo, hi + 1)
    return bool((prefix[i + k] - prefix[i] == k).any())


def _order(reads, k: int, seed: int) -> list:
    """the three copies' read order.  The permutation of the third copy is the first of a seeded series under which, at EVERY
    shift 0 .. 31, a valid k-mer crosses character 4096 * 32 and another crosses a multiple of 512 * 32 that is no chunk boundary."""
    n = len(reads)
    head = list(range(n)) + list(range(n - 1, -1, -1))
    for attempt in range(1000):
        order = head + list(np.random.RandomState(7919 * seed + 31 * k + attempt).permutation(n))
        prefix = _valid_prefix(b"".join(reads[i] + b"N" for i in order))
        total = len(prefix) - 1
        rounds = [b for b in range(ROUND_CHARS, total, ROUND_CHARS) if b % CHUNK_CHARS]
        if all(kmer_crosses(prefix, CHUNK_CHARS - j, k) and any(kmer_crosses(prefix, b - j, k) for b in rounds) for j in range(WORD)):
            return order
    raise AssertionError("no permutation lays a k-mer across the chunk and round boundaries at every shift")


def stream_of(reads, shift: int = 0, k: int | None = None, seed: int = 0) -> Laid:
    """the corpus three times -- in order, reversed, permuted --, ``shift`` N's in front as an unnamed run.  With ``k`` the
    layout is chosen and checked for that k (from the text alone): more than 4096 + 512 words, a k-mer across the chunk boundary
    and one across a round boundary, reads of k - 1, k and k + 1 characters, row boundaries between two k-mers at every position
    of a word."""
    if k is None:
        order = list(range(len(reads))) + list(range(len(reads) - 1, -1, -1)) + list(np.random.RandomState(seed).permutation(len(reads)))
    else:
        order = _order(reads, k, seed)
    laid = [reads[i] for i in order]
    runs = ([("", b"N" * shift)] if shift else []) + [(f"r{i}", r + b"N") for i, r in enumerate(laid)]
    off = np.zeros(len(runs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) for _, t in runs])
    first = 1 if shift else 0
    n = len(reads)
    names, start, end, read_of_row, read_start = [], [], [], [], []
    for i, r in enumerate(laid):
        a, b = int(off[first + i]), int(off[first + i + 1])
        cut = a + 1 + (7 * i) % (len(r) - 1) if n <= i < 2 * n and len(r) >= 2 else None      # (the second copy: two rows per read)
        for name, x, y in ((f"r{i}", a, b),) if cut is None else ((f"r{i}", a, cut), (f"r{i}+", cut, b)):
            names.append(name); start.append(x); end.append(y); read_of_row.append(i); read_start.append(a)
    as_array = lambda v: np.array(v, dtype=np.int64)
    out = Laid(runs, b"".join(t for _, t in runs), names, as_array(start), as_array(end), laid, as_array(read_of_row), as_array(read_start))
    if k is not None:
        assert 0 <= shift < WORD
        assert out.n_words > 4096 + 512
        prefix = _valid_prefix(out.text)
        assert kmer_crosses(prefix, CHUNK_CHARS, k)
        assert any(kmer_crosses(prefix, b, k) for b in range(ROUND_CHARS, len(out.text), ROUND_CHARS) if b % CHUNK_CHARS)
        assert {k - 1, k, k + 1} <= {len(r) for r in reads}
        assert all(out.text[a:b] == r + b"N" for a, b, r in zip(off[first:-1], off[first + 1:], laid))
        # row boundaries inside records: cuts with a k-mer ending on either side, at every position of a word
        inside = [int(c) for c, a0 in zip(out.start, out.read_start) if c > a0 and c >= k and prefix[c + 1] - prefix[c - k] == k + 1]
        assert len(inside) >= 100 and {c % WORD for c in inside} == set(range(WORD))
    return out


def n_reads_with_a_kmer(laid: Laid, k: int) -> int:
    """reads that hold at least one k-mer of upper-case bases: each gives the kernels at least one record"""
    n = 0
    for r in laid.reads:
        p = _valid_prefix(r)
        n += len(r) >= k and bool((p[k:] - p[:-k] == k).any())
    return n


def mini_geometry(k: int) -> tuple:
    """(M, W, delay, cap) of the minimizer scheme at this k (pg_device.hpp: mini_m, mini_window; mini.hip: mini_cap): M-mers of
    13 characters from k = 16 on and of 11 below, a window of the W <= 9 central M-mers that ends ``delay`` characters before the
    k-mer does, at most ``cap`` k-mers per record (what fits a word, the 4-bit length field, the window)"""
    m = 13 if k >= 16 else 11
    w = k - m + 1
    wc = w if w <= 9 else 8 + (w & 1)
    return m, wc, (w - wc) // 2, min(33 - k, 16, wc)


def count_records(laid: Laid, k: int, cap: int | None = None) -> tuple:
    """(records, records of more than four k-mers) of the stream under the strict plane, counted position by position the way
    the header of mini.hip defines them: a record is a maximal run of consecutive valid k-mers inside one 32-character word that
    share their minimizer value and their row, cut after ``cap`` k-mers.  The minimizer value of a k-mer is the smallest
    mhash(canonical M-mer) over its window (pg_device.hpp: mhash; codes A0 C1 T2 G3, newest character in the low bits)."""
    m, wc, delay, cap_k = mini_geometry(k)
    cap = cap_k if cap is None else min(cap, cap_k)
    t = np.frombuffer(laid.text, dtype=np.uint8)
    n = len(t)
    code = np.zeros(n + m, dtype=np.int64)                        # (m characters of padding in front)
    for ch, v in zip(b"ACTG", range(4)):
        code[m:][t == ch] = v
    fw = np.zeros(n, dtype=np.int64)
    rc = np.zeros(n, dtype=np.int64)
    for i in range(m):                                           # the M-mer that ends at q, and its reverse complement
        fw |= code[m - i:m - i + n] << (2 * i)
        rc |= (code[i + 1:i + 1 + n] ^ 2) << (2 * i)
    h = (((np.minimum(fw, rc) ^ 0x5E3779) & 0xFFFFFF) * 0xC2B2AF) & 0xFFFFFFFF
    h = np.concatenate([np.zeros(wc + delay, dtype=np.int64), h])
    mv = np.min([h[wc + delay - d:wc + delay - d + n] for d in range(delay, delay + wc)], axis=0)
    prefix = _valid_prefix(laid.text)
    ok = np.zeros(n, dtype=bool)
    ok[k - 1:] = prefix[k:] - prefix[:-k] == k
    cut = np.zeros(n + 1, dtype=bool)
    cut[laid.start] = True
    cut[laid.end] = True
    same = np.zeros(n, dtype=bool)
    same[1:] = ok[1:] & ok[:-1] & ~cut[1:n] & (mv[1:] == mv[:-1]) & (np.arange(1, n) % WORD != 0)
    n_records = n_long = length = 0
    for is_ok, goes_on in zip(ok.tolist(), same.tolist()):
        if is_ok and goes_on and length < cap:
            length += 1
            continue
        n_long += length > 4
        length = 0
        if is_ok:
            n_records += 1
            length = 1
    return n_records, n_long + (length > 4)


def check_against_oracle(laid: Laid, k: int, table) -> None:
    """what the expected values rest on, from the oracle's table of ``laid.text``: no count near the packed tables' saturation
    value, counts on both sides of 64 (so that window 1, vsize 64 drops some), and for even k a k-mer that is its own reverse
    complement"""
    from oracle import oracle
    from pangaea_amd import _lib
    codes, counts = table.items()
    assert 64 < int(counts.max()) < _lib.HASH_COUNT_SAT // 256 and int(counts.min()) < 64
    if k % 2 == 0:
        assert any(oracle.revcomp(int(c), k) == int(c) for c in codes)
