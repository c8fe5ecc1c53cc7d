"""An edge-case read corpus for the super-k-mer kernels (pangaea_amd/csrc/mini.hip), built for one k from a seeded random base
sequence -- what ``synth.generate`` never produces: reads shorter than k, an N or a soft-masked base at every position of a
word, periodic reads that reach the record cap, palindromic M-mers and k-mers, and every read's reverse complement.

``corpus(k, seed)`` is the list of reads (bytes, no separator).  ``stream_of(reads, shift, k)`` lays it out three times (in order,
reversed, in a seeded permutation), every read followed by ``N`` and a run of its own -- and a row of its own, or two in the
second copy, whose row boundaries lie inside records --, behind ``shift`` N's that move the whole text against the 32-character
word grid.  ``check_against_oracle`` makes the assertions that need the oracle's table.
``masked_corpus`` / ``masked_stream_of`` add low-quality marks (a mask beside the text) and reads without a row, ``shard`` cuts a
layout for one of N ranks: the second half of this file, for the N-rank form.
A plain module: the host test (tests/test_mini_corpus_host.py) checks it at every k, the GPU tests (tests/test_mini_corpus_gpu.py on
one GPU, tests/test_dist_corpus_gpu.py on N ranks) run the kernels on it."""
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


def _kmer_ends(text: bytes, k: int) -> np.ndarray:
    """per character: does a k-mer of upper-case bases END there?"""
    prefix = _valid_prefix(text)
    ok = np.zeros(len(text), dtype=bool)
    ok[k - 1:] = prefix[k:] - prefix[:-k] == k
    return ok


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


def count_records(laid, k: int, cap: int | None = None, planes: tuple | None = None) -> tuple:
    """(records, records of more than four k-mers) of the stream under the strict plane, counted position by position the way
    the header of mini.hip defines them: a record is a maximal run of consecutive valid k-mers inside one 32-character word that
    share their minimizer value and their row, cut after ``cap`` k-mers.  The minimizer value of a k-mer is the smallest
    mhash(canonical M-mer) over its window (pg_device.hpp: mhash; codes A0 C1 T2 G3, newest character in the low bits).
    ``planes`` = (kept, T, R) of ``kmer_planes``: the MASKED rule (include/pangaea_feat.h, the block before pg_mini_plan_masked)
    -- the kept k-mers take the place of the valid ones, and records are also cut where T or R changes; the characters are
    then read without their case (a soft-masked base is a base of the table's plane)."""
    m, wc, delay, cap_k = mini_geometry(k)
    cap = cap_k if cap is None else min(cap, cap_k)
    t = np.frombuffer(laid.text if planes is None else laid.text.upper(), dtype=np.uint8)
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
    cut = np.zeros(n + 1, dtype=bool)
    cut[laid.start] = True
    cut[laid.end] = True
    if planes is None:
        ok = _kmer_ends(laid.text, k)
    else:
        ok, in_table, in_rows = planes
        cut[1:n] |= (in_table[1:] != in_table[:-1]) | (in_rows[1:] != in_rows[:-1])
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


# ------------------------------------------------------------------ masks and shards: the corpus for the N-rank form
#
# dist.MiniSharded counts a rank's shard of the stream (dist.shard_stream: a range of runs, cut out of the words it shares with
# its neighbours) under TWO planes where the input is masked: T, the table's (bases below the quality threshold are no bases, and
# with ``lowercase_is_base`` soft-masked bases are), and R, the rows' strict one (include/pangaea_feat.h, the block before
# pg_mini_plan_masked).  ``masked_corpus`` adds reads with low-quality marks to ``corpus``, ``masked_stream_of`` lays them out
# with the mask beside the text, ``shard`` cuts a layout (masked or plain) for a rank.

ROWLESS_THIRD, ROWLESS_OTHER = 5, 17     # every fifth read of the third copy has no row, every 17th of the first two
COPIES = (0, 1, 2)


@dataclass(frozen=True)
class Marked:
    """a read, the offsets of its low-quality marks (always on bases), the copies of the layout in which it carries them
    and the copies that hold it at all"""
    text: bytes
    marks: tuple = ()
    marked_in: tuple = COPIES
    laid_in: tuple = COPIES

    def revcomp(self) -> "Marked":
        return Marked(revcomp(self.text), tuple(sorted(len(self.text) - 1 - m for m in self.marks)), self.marked_in, self.laid_in)


def _flank(rng, n: int) -> bytes:
    """random text that neither begins nor ends with A or T: it does not lengthen a run of A or of T beside it"""
    return b"C" + _random(rng, n - 2) + b"G"


def _lower(read: bytes, a: int, b: int) -> bytes:
    return read[:a] + read[a:b].lower() + read[b:]


def clean_poly_a(k: int) -> bytes:
    return b"A" * max(70, k + 49)


def masked_corpus(k: int, seed: int = 0, clean_run: bool = True) -> list:
    """the reads of ``corpus(k, seed)`` -- unmarked, but for the two that hold the all-A k-mer (the period-1 read and its reverse
    complement), which are marked every k - 1 characters: with them clean, every rank would count the k-mer of code 0 -- and
    four families of marked reads, each with its reverse complements:
    (g) a base read of 96 characters 96 times, copy j marked at offset j, in the first two copies of the layout only;
    (h) reads of k .. k + 5 characters marked in the middle: no clean stretch reaches k, nobody counts their k-mers;
    (i) runs of A and of T of k + 3k/7 and k + 4k/21 characters, marked in the middle, between random text; and, with
        ``clean_run``, ONE clean run of A in the third copy only: the one place where the all-A k-mer is counted;
    (j) reads with a lower-case stretch and marks: adjacent, overlapping (a low-quality lower-case base is a base of neither
        plane) and fewer than k characters apart."""
    rng = np.random.RandomState(1000 * seed + k + 500)
    out = []
    for r in corpus(k, seed):
        poly = b"A" * k in r or b"T" * k in r
        out.append(Marked(r, tuple(range(k // 2, len(r), k - 1)) if poly else ()))
    base = _random(rng, BASE_LEN)
    new = [Marked(base, (j,), (0, 1)) for j in range(BASE_LEN)]                                  # (g)
    for n in range(k, k + 6):                                                                    # (h)
        new.append(Marked(_random(rng, n), (n // 2,)))
    a, c = k + 3 * k // 7, k + 4 * k // 21
    for _ in range(3):                                                                           # (i)
        body = _flank(rng, 120) + b"A" * a + _flank(rng, 80) + b"T" * a + _flank(rng, 60) + b"A" * c + _flank(rng, 40)
        new.append(Marked(body, (120 + a // 2, 120 + a + 80 + a // 2 - 1, 120 + a + 80 + a + 60 + c // 2)))
    for s in (20, 31, 45, 58):                                                                   # (j)
        r = _random(rng, BASE_LEN)
        new.append(Marked(_lower(r, s, s + 3), (s + 3,)))                                        # adjacent
        new.append(Marked(_lower(r, s, s + 4), (s + 2, s + 3, s + 4, s + 5)))                    # overlapping
        new.append(Marked(_lower(r, s, s + 2), (s + 2 + k // 2,)))                               # fewer than k apart
    out += new + [m.revcomp() for m in new]
    if clean_run:
        out.append(Marked(clean_poly_a(k), laid_in=(2,)))
    for m in out:
        assert all(m.text[i:i + 1].upper() in (b"A", b"C", b"G", b"T") for i in m.marks)
    return out


def plane_of(mask: np.ndarray, n_words: int):
    """a per-character boolean mask as a plane of the stream (bit j of word w = character 32 w + j), a torch tensor"""
    import torch
    m = np.zeros(n_words * WORD, dtype=np.uint64)
    m[:mask.size] = mask
    bits = (m.reshape(n_words, WORD) << np.arange(WORD, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return torch.from_numpy(bits.view(np.int32).copy())


@dataclass
class MaskedLaid(Laid):
    """a masked corpus laid out: ``text`` is the STRICT text (what the rows see: the oracle takes a lower-case character for
    no base), ``lowq`` the low-quality mask beside it, per character"""
    lowq: np.ndarray = None

    def table_text(self, lowercase_is_base: bool = False) -> bytes:
        """what the table counts: low-quality characters are N, and soft-masked bases are bases with ``lowercase_is_base``"""
        t = np.frombuffer(self.text.upper() if lowercase_is_base else self.text, dtype=np.uint8).copy()
        t[self.lowq] = ord("N")
        return t.tobytes()


def masked_stream_of(marked, shift: int, k: int, seed: int = 0) -> MaskedLaid:
    """the masked corpus three times -- in order, reversed, in a seeded permutation; every read in the copies it is laid in, its
    marks in the copies it is marked in --, ``shift`` N's in front as an unnamed run, every read followed by N and a run of
    its own.  Rows as in ``stream_of`` (one per read, two in the second copy), except that every ``ROWLESS_THIRD``-th read of the
    third copy and every ``ROWLESS_OTHER``-th of the first two has NO row: a k-mer that only the rows' plane keeps is dropped there
    (with three ranks every rank holds one copy, so each copy needs such reads)."""
    per_copy = [[m for m in marked if c in m.laid_in] for c in COPIES]
    perm = np.random.RandomState(7919 * seed + 31 * k + 5).permutation(len(per_copy[2]))
    laid = ([(m, 0) for m in per_copy[0]] + [(m, 1) for m in reversed(per_copy[1])] + [(per_copy[2][i], 2) for i in perm])
    runs = ([("", b"N" * shift)] if shift else []) + [(f"r{i}", m.text + b"N") for i, (m, _) in enumerate(laid)]
    off = np.zeros(len(runs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) for _, t in runs])
    first = 1 if shift else 0
    lowq = np.zeros(int(off[-1]), dtype=bool)
    names, start, end, read_of_row, read_start = [], [], [], [], []
    for i, (m, copy) in enumerate(laid):
        a, b = int(off[first + i]), int(off[first + i + 1])
        if copy in m.marked_in and m.marks:
            lowq[a + np.array(m.marks)] = True
        if i % (ROWLESS_THIRD if copy == 2 else ROWLESS_OTHER) == (ROWLESS_THIRD if copy == 2 else ROWLESS_OTHER) - 1:
            continue
        cut = a + 1 + (7 * i) % (len(m.text) - 1) if copy == 1 and len(m.text) >= 2 else None
        for name, x, y in ((f"r{i}", a, b),) if cut is None else ((f"r{i}", a, cut), (f"r{i}+", cut, b)):
            names.append(name); start.append(x); end.append(y); read_of_row.append(i); read_start.append(a)
    as_array = lambda v: np.array(v, dtype=np.int64)
    text = b"".join(t for _, t in runs)
    t = np.frombuffer(text.upper(), dtype=np.uint8)
    assert np.isin(t[lowq], list(b"ACGT")).all() and 0 <= shift < WORD
    return MaskedLaid(runs, text, names, as_array(start), as_array(end), [m.text for m, _ in laid], as_array(read_of_row),
                      as_array(read_start), lowq)


def kmer_planes(strict_text: bytes, table_text: bytes, start, end, k: int) -> tuple:
    """(kept, T, R, inside a row) per character, for the k-mer that ENDS there: T -- its characters are bases of the table's text;
    R -- of the strict text; a k-mer lies in the row that holds its last character; kept if T holds, or R inside a row"""
    in_table, in_rows = _kmer_ends(table_text, k), _kmer_ends(strict_text, k)
    inside = np.zeros(len(strict_text), dtype=bool)
    for a, b in zip(start, end):
        inside[a:b] = True
    return in_table | (in_rows & inside), in_table, in_rows, inside


def kmers_at(text: bytes, ends: np.ndarray, k: int) -> bytes:
    """the k-mers that end at these characters, N between them: a text for ``oracle.Table`` that holds exactly these"""
    return b"N".join(text[p - k + 1:p + 1] for p in ends.tolist())


def run_cuts(laid, world: int) -> list:
    """the characters at which ``dist.shard_stream`` cuts the stream for ``world`` ranks (dist.balanced_run_ranges: at run
    boundaries), from the layout alone; [0, .., len(text)]"""
    run_off = np.zeros(len(laid.runs) + 1, dtype=np.int64)
    run_off[1:] = np.cumsum([len(t) for _, t in laid.runs])
    n = len(laid.runs)
    cuts = [0]
    for r in range(1, world):
        i = int(np.searchsorted(run_off, run_off[-1] * r // world, side="left"))
        cuts.append(min(max(i, cuts[-1]), n))
    return [int(run_off[i]) for i in cuts] + [int(run_off[-1])]


def cuts_are_partial(laid, k: int, worlds=(2, 3)) -> list:
    """does the layout make ``dist._cut_plane`` mask bits on every rank of every world -- no cut on a word boundary, the text no
    whole number of words?  Then: the worlds with a cut that has a whole k-mer of the table's text between the start of the
    cut's word and the cut -- characters of the rank before, which the next rank would count AGAIN if it did not mask them (a
    cut behind fewer than k bases shows no such mistake: in the plain layout the world-2 cut lies among the shortest reads of
    the reversed copy).  An empty list: no."""
    table_text = laid.table_text() if isinstance(laid, MaskedLaid) else laid.text
    ok = _kmer_ends(table_text, k)
    inner = {world: run_cuts(laid, world)[1:-1] for world in worlds}
    if len(laid.text) % WORD == 0 or any(c % WORD == 0 for cuts in inner.values() for c in cuts):
        return []
    return [world for world, cuts in inner.items() if any(ok[c - c % WORD + k - 1:c].any() for c in cuts)]


def sharded_layout(k: int, masked: bool, seed: int = 0, clean_run: bool = True):
    """the corpus (``masked``: the masked one) laid out at the smallest odd shift under which ``cuts_are_partial`` holds"""
    reads = masked_corpus(k, seed, clean_run) if masked else corpus(k, seed)
    for shift in range(1, WORD, 2):
        laid = masked_stream_of(reads, shift, k, seed) if masked else stream_of(reads, shift, k, seed)
        if cuts_are_partial(laid, k):
            return laid
    raise AssertionError("no odd shift makes the first and the last word of every shard partial")


@dataclass
class Shard:
    """a rank's part of a layout: the host stream ``dist.shard_stream`` cuts, its rows in the shard's own coordinates, and
    the same in Python -- the shard's strict text and low-quality mask from its first WORD on (the characters of the rank
    before, which share that word, are N's), for the oracle and ``kmer_planes``"""
    stream: object
    rows: object
    row_range: tuple           # the rows of the layout that are this rank's: [first, last)
    char_range: tuple          # the characters of the layout that are this rank's
    lo: int                    # the rank's first character in its first word
    hi: int                    # one past its last character in its last word (WORD: the word is whole)
    text: bytes
    lowq: np.ndarray
    reads: list

    def table_text(self, lowercase_is_base: bool = False) -> bytes:
        t = np.frombuffer(self.text.upper() if lowercase_is_base else self.text, dtype=np.uint8).copy()
        t[self.lowq] = ord("N")
        return t.tobytes()


def host_stream(laid, quality: bool = True):
    """the layout as a host ``ReadStream``, its low-quality plane beside it (``quality``; a plain layout has none)"""
    from pangaea_amd.reads import ReadStream
    s = ReadStream.from_runs(laid.runs)
    assert s.n_chars == len(laid.text)
    if quality and isinstance(laid, MaskedLaid):
        s.valid_lowq = plane_of(laid.lowq, s.n_words)
    return s


def shard(laid, world: int, rank: int, quality: bool = True) -> Shard:
    """(``world``, ``rank``) -> the rank's ``ReadStream``, cut by ``dist.shard_stream`` from the host stream with its planes, and its
    ``Rows``: those of the layout that lie in the rank's run range, moved by the shard's word offset.  ``quality=False``: the
    shard without its low-quality plane (a rank whose input has none)."""
    from pangaea_amd import dist
    from pangaea_amd.reads import Rows
    s = host_stream(laid, quality)
    first, last = dist.balanced_run_ranges(s.run_off, world)[rank]
    cuts = run_cuts(laid, world)
    c0, c1 = cuts[rank], cuts[rank + 1]
    assert c0 == int(s.run_off[first]) and c1 == (int(s.run_off[last]) if rank < world - 1 else s.n_chars)
    part = dist.shard_stream(s, rank, world)
    w0 = c0 // WORD
    rows = laid.rows()
    mine = np.flatnonzero((rows.run_index >= first) & (rows.run_index < last))
    assert len(mine) and (np.diff(mine) == 1).all()
    assert (rows.start[mine] >= c0).all() and (rows.end[mine] <= c1).all()                     # (a read is a run: no row straddles a cut)
    local = Rows(rows.run_index[mine] - first, [rows.names[i] for i in mine], rows.start[mine] - WORD * w0, rows.end[mine] - WORD * w0)
    lo, hi = c0 - WORD * w0, c1 - WORD * ((c1 + WORD - 1) // WORD - 1)
    lowq = np.zeros(c1 - WORD * w0, dtype=bool)
    if quality and isinstance(laid, MaskedLaid):
        lowq[lo:] = laid.lowq[c0:c1]
    n_before = (1 if laid.runs[0][0] == "" else 0)
    reads = laid.reads[max(0, first - n_before):last - n_before]
    assert part.n_chars == c1 - WORD * w0 and len(part.run_names) == last - first
    return Shard(part, local, (int(mine[0]), int(mine[-1]) + 1), (c0, c1), lo, hi, b"N" * lo + laid.text[c0:c1], lowq, reads)
