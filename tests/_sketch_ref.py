"""A plain numpy restatement of the HyperLogLog sizing sketch (include/pangaea_feat.h, the comment of ``pg_kmer_distinct_sketch``),
for the tests to compare with.  Nothing here is shared with the code under test; it imports without a GPU.

  k-mers     every character p of [char_begin, char_end) that ENDS a run of at least k valid characters gives the k-mer
             text[p - k + 1 .. p]: it belongs to the range its LAST character lies in, wherever it starts
  valid      upper-case ACGT; with ``lowercase_is_base`` lower-case acgt too; with ``plane`` the set bits of the plane alone
             (bit j of word w = character 32 w + j), the characters then read without their case
  code       A0 C1 T2 G3, the newest base in the low bits; complement = c ^ 2; canonical = min(forward, reverse complement)
  hash       h = mix64(code ^ 0x9E3779B97F4A7C15), mix64 = xorshift 33, multiply, twice, xorshift 33 (pg_device.hpp)
  register   idx = h >> 52; rank = clz64((h << 12) | (1 << 11)) + 1, 1 .. 53; registers[idx] = max(registers[idx], rank)
  estimate   alpha m^2 / sum_j 2^-registers[j], alpha = 0.7213 / (1 + 1.079 / m); m ln(m / V) instead where that is at most
             2.5 m and V > 0 registers are zero; truncated to an integer

All arithmetic on codes and hashes is uint64 in numpy arrays (which wrap silently); leading zeros are counted by shifting.

``fault=`` on ``kmers_of_text``, ``registers_of_codes`` and ``combine`` switches ONE deliberate mistake into the reference
(``FAULTS``): tests/test_sketch_host.py shows, on the CPU, that each of them changes the registers of the input that
tests/test_sketch_gpu.py runs the kernel on -- a kernel with that mistake would fail there.  The second half of this file builds
those inputs, for both test files."""
import functools

import numpy as np

WORD = 32
HLL_BITS = 12
M = 1 << HLL_BITS
XOR = 0x9E3779B97F4A7C15
MUL1, MUL2 = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53
MAX_RANK = 64 - HLL_BITS + 1                                    # 53: the sentinel bit below the 52 hash bits ends every run of zeros

FAULTS = {"forward": "(a) the forward code where the canonical one was meant",
          "drop-straddlers": "(b) k-mers that start before the range dropped",
          "own-by-start": "(c) a k-mer owned by the range it STARTS in",
          "short-run": "(d) a run of k - 1 valid characters accepted",
          "no-xor": "(e) the xor constant omitted",
          "low-index": "(f) the index taken from the low 12 bits of the hash",
          "rank-minus-one": "(g) the rank without its + 1",
          "no-sentinel": "(h) no sentinel bit: the rank runs up to 65",
          "sentinel-high": "(i) the sentinel one bit higher",
          "code32": "(j) the code truncated to 32 bits",
          "overwrite": "(k) two sketches combined by overwriting, not by max"}
_TEXT_FAULTS = ("forward", "drop-straddlers", "own-by-start", "short-run")
_CODE_FAULTS = ("no-xor", "low-index", "rank-minus-one", "no-sentinel", "sentinel-high", "code32")


def _u64(x) -> np.ndarray:
    return np.atleast_1d(np.asarray(x, dtype=np.uint64)).copy()


def mix64(x) -> np.ndarray:
    x = _u64(x)
    for mul in (MUL1, MUL2):
        x ^= x >> np.uint64(33)
        x *= np.uint64(mul)
    x ^= x >> np.uint64(33)
    return x


def mix64_inverse(h) -> np.ndarray:
    """``x ^= x >> 33`` is an involution on 64 bits (it changes the low 31 bits by the top 31, which it leaves as they are); the
    odd multipliers have inverses modulo 2^64"""
    x = _u64(h)
    for mul in (MUL2, MUL1):
        x ^= x >> np.uint64(33)
        x *= np.uint64(pow(mul, -1, 1 << 64))
    x ^= x >> np.uint64(33)
    return x


def clz64(x) -> np.ndarray:
    """leading zeros of every uint64 (64 for 0), by shifting"""
    x = _u64(x)
    zero = x == 0
    n = np.zeros(x.shape, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        top_clear = (x >> np.uint64(64 - s)) == 0
        n[top_clear] += s
        x[top_clear] <<= np.uint64(s)
    n[zero] = 64
    return n


def revcomp_codes(codes, k: int) -> np.ndarray:
    c = _u64(codes)
    out = np.zeros(c.shape, dtype=np.uint64)
    for _ in range(k):
        out = (out << np.uint64(2)) | ((c & np.uint64(3)) ^ np.uint64(2))
        c >>= np.uint64(2)
    return out


def canonical_of(codes, k: int) -> np.ndarray:
    c = _u64(codes)
    return np.minimum(c, revcomp_codes(c, k))


def kmer_of_code(code: int, k: int) -> bytes:
    return bytes(b"ACTG"[(int(code) >> (2 * (k - 1 - j))) & 3] for j in range(k))


def code_of_kmer(kmer: bytes) -> int:
    code = 0
    for ch in kmer:
        code = (code << 2) | b"ACTG".index(ch)
    return code


def plane_bits(plane, n_chars: int) -> np.ndarray:
    """a plane of the stream (int32 or uint32 words, bit j of word w = character 32 w + j) as one bool per character"""
    words = np.ascontiguousarray(np.asarray(plane)).view(np.uint32)
    bits = (words[:, None] >> np.arange(WORD, dtype=np.uint32)[None, :]) & np.uint32(1)
    return bits.reshape(-1)[:n_chars].astype(bool)


def kmers_of_text(text: bytes, k: int, plane=None, lowercase_is_base: bool = False, char_begin: int = 0, char_end=None,
                  fault=None) -> tuple:
    """(end positions, canonical codes) of the k-mers that end in [char_begin, char_end), in text order, repeats included"""
    assert 1 <= k <= 31 and fault in (None,) + _TEXT_FAULTS and (k > 1 or fault != "short-run")
    n = len(text)
    char_end = n if char_end is None else char_end
    raw = np.frombuffer(text, dtype=np.uint8)
    if plane is not None:
        valid = plane_bits(plane, n)
        valid = np.concatenate([valid, np.zeros(n - len(valid), dtype=bool)])
    else:
        valid = np.isin(raw, list(b"ACGTacgt" if lowercase_is_base else b"ACGT"))
    code = np.zeros(n + k, dtype=np.uint64)                      # (k characters of padding in front, code 0 like every non-base)
    for ch, v in zip(b"ACTGactg", (0, 1, 2, 3) * 2):
        code[k:][raw == ch] = v
    code[k:][~valid] = 0
    run = k - 1 if fault == "short-run" else k
    prefix = np.concatenate([[0], np.cumsum(valid)])
    ends = np.flatnonzero(prefix[run:] - prefix[:n + 1 - run] == run) + run - 1 if n >= run else np.zeros(0, dtype=np.int64)
    own = ends - k + 1 if fault == "own-by-start" else ends
    keep = (own >= char_begin) & (own < char_end)
    if fault == "drop-straddlers":
        keep &= ends - k + 1 >= char_begin
    ends = ends[keep]
    fw = np.zeros(len(ends), dtype=np.uint64)
    rc = np.zeros(len(ends), dtype=np.uint64)
    for i in range(k):                                           # character ends - i: digit i of the forward code, k - 1 - i of the other
        c = code[k + ends - i]
        fw |= c << np.uint64(2 * i)
        rc |= (c ^ np.uint64(2)) << np.uint64(2 * (k - 1 - i))
    return ends, (fw if fault == "forward" else np.minimum(fw, rc))


def canonical_codes(text: bytes, k: int, plane=None, lowercase_is_base: bool = False) -> np.ndarray:
    """the distinct canonical codes of the text, sorted: what ``oracle.Table(k).count(text).items()[0]`` holds"""
    return np.unique(kmers_of_text(text, k, plane, lowercase_is_base)[1])


def index_and_rank(codes, fault=None) -> tuple:
    assert fault in (None,) + _CODE_FAULTS
    c = _u64(codes)
    if fault == "code32":
        c &= np.uint64(0xFFFFFFFF)
    h = mix64(c if fault == "no-xor" else c ^ np.uint64(XOR))
    idx = (h & np.uint64(M - 1)) if fault == "low-index" else (h >> np.uint64(64 - HLL_BITS))
    sentinel = {"no-sentinel": 0, "sentinel-high": 1 << HLL_BITS}.get(fault, 1 << (HLL_BITS - 1))
    rank = clz64((h << np.uint64(HLL_BITS)) | np.uint64(sentinel)) + (0 if fault == "rank-minus-one" else 1)
    return idx.astype(np.int64), rank


def registers_of_codes(codes, fault=None) -> np.ndarray:
    """int64 [4096]; the registers depend on the SET of codes alone"""
    idx, rank = index_and_rank(codes, fault)
    regs = np.zeros(M, dtype=np.int64)
    np.maximum.at(regs, idx, rank)
    return regs


def registers_of_text(text: bytes, k: int, char_begin: int = 0, char_end=None, plane=None, lowercase_is_base: bool = False,
                      fault=None) -> np.ndarray:
    text_fault = fault if fault in _TEXT_FAULTS else None
    codes = kmers_of_text(text, k, plane, lowercase_is_base, char_begin, char_end, text_fault)[1]
    return registers_of_codes(codes, None if text_fault else fault)


def combine(a: np.ndarray, b: np.ndarray, fault=None) -> np.ndarray:
    """the sketch of a union from the sketches of its parts (``b`` arriving second)"""
    assert fault in (None, "overwrite")
    return np.where(b != 0, b, a) if fault else np.maximum(a, b)


def estimate(regs) -> int:
    r = np.asarray(regs).astype(np.int64)
    m = len(r)
    held = np.bincount(r, minlength=1)
    total = 0.0
    for value in range(len(held) - 1, -1, -1):                   # (the smallest terms first)
        total += float(held[value]) * 2.0 ** -value
    est = 0.7213 / (1.0 + 1.079 / m) * m * m / total
    zeros = int(held[0])
    if est <= 2.5 * m and zeros:
        est = m * float(np.log(m / zeros))
    return int(est)


def kmer_with(idx: int, rank: int, k: int = 31) -> bytes:
    """a k-mer whose register is ``idx`` -- or the first one after it, cyclically, that has such a k-mer -- and whose rank is
    ``rank``: the hash h = idx << 52 | 1 << (52 - rank) (nothing below the 52 bits for rank 53) inverted.
    mix64^-1(h) ^ constant is a canonical k-mer's code if it lies below 4^k and not above its reverse complement: at k = 31
    for about one register in eight.  ``index_and_rank(code_of_kmer(..))`` tells which register it became."""
    assert 0 <= idx < M and 1 <= rank <= MAX_RANK and 1 <= k <= 31
    low = 0 if rank == MAX_RANK else 1 << (64 - HLL_BITS - rank)
    walk = (np.arange(M, dtype=np.uint64) + np.uint64(idx)) % np.uint64(M)
    codes = mix64_inverse((walk << np.uint64(64 - HLL_BITS)) | np.uint64(low)) ^ np.uint64(XOR)
    fits = codes < np.uint64(1 << (2 * k))
    fits &= codes <= revcomp_codes(np.where(fits, codes, np.uint64(0)), k)
    if not fits.any():
        raise ValueError(f"no canonical {k}-mer of rank {rank} in any register")
    return kmer_of_code(int(codes[np.argmax(fits)]), k)


# ------------------------------------------------------------------ the inputs of tests/test_sketch_gpu.py
#
# Built here, from seeded generators, so that tests/test_sketch_host.py can show on the CPU what each of them discriminates.

RANGE_WORDS = 4096
RANGE_CUTS = (1, 255, 256, 1023, 1024, 1025, 4095)
CONTENDED_WORDS = 1 << 15
BLOCK_WORDS = 1024                                              # words per workgroup and trip of the kernel
TRIP_WORDS = (1 << 20) + 2048                                   # 1024 workgroups of 1024 words: one trip; this takes a second one
ISLAND = 300
EXTREME_RANKS = (1, 2, 33, 52, 53)
RANK53 = b"ACAGAGCGTGAGTTATTGTTGAACGCGAGGC"
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(read: bytes) -> bytes:
    return read.translate(_COMP)[::-1]


def random_bases(rng, n: int) -> np.ndarray:
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, size=n)]


@functools.lru_cache(maxsize=None)
def range_text() -> bytes:
    """4096 words of random bases (one strand: no k-mer's reverse complement is there but by chance) with an N about every 200
    characters"""
    rng = np.random.RandomState(4096)
    t = random_bases(rng, RANGE_WORDS * WORD).copy()
    t[rng.rand(len(t)) < 1 / 200] = ord("N")
    return t.tobytes()


@functools.lru_cache(maxsize=None)
def contended_text() -> bytes:
    """2^15 words of random bases: 32 workgroups, about 256 k-mers per register"""
    return random_bases(np.random.RandomState(15), CONTENDED_WORDS * WORD).tobytes()


def island_starts() -> tuple:
    """where the islands of ``trip_text`` begin: character 0, across the word boundaries 1023 | 1024, 2^20 - 1 | 2^20 and
    2^20 + 1023 | 2^20 + 1024, and at the very end"""
    across = [w * WORD - ISLAND // 2 for w in (1024, 1 << 20, (1 << 20) + 1024)]
    return (0, *across, TRIP_WORDS * WORD - ISLAND)


def trip_islands() -> list:
    rng = np.random.RandomState(20)
    return [random_bases(rng, ISLAND).tobytes() for _ in island_starts()]


def trip_text() -> np.ndarray:
    """2^20 + 2048 words of N (uint8, 34 MB) but for the islands"""
    t = np.full(TRIP_WORDS * WORD, ord("N"), dtype=np.uint8)
    for at, island in zip(island_starts(), trip_islands()):
        t[at:at + ISLAND] = np.frombuffer(island, dtype=np.uint8)
    return t


@functools.lru_cache(maxsize=None)
def extreme_kmers() -> tuple:
    """31-mers of the ranks 1, 2, 33, 52 and 53 in registers of their own, and the reverse complements of two of them"""
    kmers = [kmer_with(700 * i + 5, r) for i, r in enumerate(EXTREME_RANKS)]
    assert kmers[-1] != RANK53
    kmers.append(RANK53)
    return tuple(kmers + [revcomp(kmers[2]), revcomp(RANK53)])


def extreme_text(shift: int) -> bytes:
    return b"N" * shift + b"N".join(extreme_kmers()) + b"N"


def repeat_text(unit: bytes, n_words: int = 2048) -> bytes:
    return (unit * (n_words * WORD // len(unit) + 1))[:n_words * WORD]


def thinned(valid_words, seed: int = 2, fraction: float = 0.02) -> np.ndarray:
    """the plane with a seeded ``fraction`` of its set bits cleared (uint32 words)"""
    words = np.ascontiguousarray(np.asarray(valid_words)).view(np.uint32)
    bits = plane_bits(words, len(words) * WORD)
    drop = np.flatnonzero(bits)
    drop = drop[np.random.RandomState(seed).rand(len(drop)) < fraction]
    bits[drop] = False
    return (bits.reshape(-1, WORD).astype(np.uint32) << np.arange(WORD, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)


def distinct_canonical(k: int, n: int, seed: int) -> np.ndarray:
    """``n`` distinct canonical k-mer codes in the order a seeded generator draws them (every prefix is a draw of its own)"""
    rng = np.random.RandomState(1000 * seed + k)
    want = min(int(1.6 * n) + 64, 4 * n + 64)
    raw = rng.randint(0, 1 << 62, size=want, dtype=np.int64).astype(np.uint64) >> np.uint64(62 - 2 * k)
    canon = canonical_of(raw, k)
    _, first = np.unique(canon, return_index=True)
    first.sort()
    assert len(first) >= n, (k, n, len(first))
    return canon[first[:n]]
