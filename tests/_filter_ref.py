"""A plain numpy / Python restatement of ``KmerTable.read_hits`` and ``KmerTable.filter_fastq`` (include/pangaea_feat.h, "Reads of a
FASTQ text by their k-mers' counts"), for the tests to compare with.  Nothing here is shared with the code under test.

  lines      a line ends at ``\\n``; a last line without one is a line; ``\\r`` is an ordinary byte of its line
  records    record r is lines 4r .. 4r + 3; line 0 begins with ``@``, line 2 with ``+``; a line count that is no multiple of 4
             is malformed at record ``lines // 4``; with ``min_qual_char`` a quality line shorter than its sequence line is too
  k-mers     position i of the sequence line holds one iff i + k <= length and bytes i .. i + k - 1 are all bases: ACGT, acgt
             too under ``lowercase_is_base``; with ``min_qual_char`` a base whose quality byte is below it is no base
  hits       n = the record's k-mers, h = those whose count c in the table (0: absent) has lower <= c <= upper
  passes     n >= 1 and h >= min_hits and h <= max_hits; an int bound is absolute, a float one a share: h >= f * n in double
  pairs      any: both mates stay if either passes; both: if both pass; single: every record on its own
"""
import numpy as np

_DIGIT = np.full(256, -1, np.int64)
_DIGIT[list(b"ACTG")] = np.arange(4)
_DIGIT_LENIENT = _DIGIT.copy()
_DIGIT_LENIENT[list(b"actg")] = np.arange(4)


class Malformed(ValueError):
    """``record``: the 0-based ordinal of the first malformed record of its file"""

    def __init__(self, record: int, why: str):
        super().__init__(f"record {record}: {why}")
        self.record = record


def lines_of(data: bytes) -> list:
    """[(start, end without the newline, end with it)] of every line"""
    out, at = [], 0
    while at < len(data):
        j = data.find(b"\n", at)
        if j < 0:
            out.append((at, len(data), len(data)))
            break
        out.append((at, j, j + 1))
        at = j + 1
    return out


def records_of(data: bytes, min_qual_char=None) -> list:
    """[(first byte, byte behind the record, sequence line, quality line)] of every record; Malformed for the first bad one"""
    lines = lines_of(data)
    recs = []
    for r in range((len(lines) + 3) // 4):
        four = lines[4 * r:4 * r + 4]
        if len(four) < 4:
            raise Malformed(r, f"the text ends inside it ({len(four)} of 4 lines)")
        l0, l1, l2, l3 = (data[a:b] for a, b, _ in four)
        if l0[:1] != b"@":
            raise Malformed(r, "its first line does not begin with '@'")
        if l2[:1] != b"+":
            raise Malformed(r, "its third line does not begin with '+'")
        if min_qual_char is not None and len(l3) < len(l1):
            raise Malformed(r, "its quality line is shorter than its sequence line")
        recs.append((four[0][0], four[3][2], l1, l3))
    return recs


def _rc(codes, k):
    c = np.asarray(codes, dtype=np.uint64).copy()
    out = np.zeros_like(c)
    for _ in range(k):
        out = (out << np.uint64(2)) | ((c & np.uint64(3)) ^ np.uint64(2))
        c >>= np.uint64(2)
    return out


def _profile(seq: bytes, qual, k: int, items, lowercase_is_base=True, min_qual_char=None) -> tuple:
    """(holds: bool, counts: int64) for positions 0 .. len - k of ``seq`` (both empty where len < k): does the position hold a
    k-mer, and the table's count of it (0: the table lacks it).  ``items``: (codes sorted, counts), as ``KmerTable.items()`` and
    ``oracle.Table.items()`` give them; ``qual``: one quality byte per byte of ``seq`` (looked at under ``min_qual_char`` only)"""
    d = (_DIGIT_LENIENT if lowercase_is_base else _DIGIT)[np.frombuffer(seq, np.uint8)]
    if min_qual_char is not None:
        d = np.where(np.frombuffer(qual, np.uint8) >= ord(min_qual_char), d, -1)
    n = len(d)
    if n < k:
        return np.zeros(0, bool), np.zeros(0, np.int64)
    bad = np.concatenate([[0], np.cumsum(d < 0)])
    m = n - k + 1
    holds = (bad[k:] - bad[:m]) == 0
    dd = np.where(d < 0, 0, d).astype(np.uint64)
    fw = np.zeros(m, np.uint64)
    for j in range(k):
        fw = (fw << np.uint64(2)) | dd[j:j + m]
    canon = np.minimum(fw, _rc(fw, k))
    codes, counts = items
    if len(codes) == 0:
        return holds, np.zeros(m, np.int64)
    at = np.minimum(np.searchsorted(codes, canon), len(codes) - 1)
    return holds, np.where(codes[at] == canon, counts[at], 0).astype(np.int64)


def kmer_counts(seq: bytes, qual: bytes, k: int, items, lowercase_is_base=True, min_qual_char=None) -> np.ndarray:
    """int64: the table's count of every k-mer of one sequence line, in order"""
    holds, counts = _profile(seq, qual[:len(seq)], k, items, lowercase_is_base, min_qual_char)
    return counts[holds]


def read_hits(data: bytes, k: int, items, lower=1, upper=None, lowercase_is_base=True, min_qual_char=None, counts_cache=None) -> np.ndarray:
    """int64 [n_records, 2]: (n, h) of every record.  The sequence lines are looked at in one piece, a newline (no base) between
    them; ``counts_cache`` (a dict) keeps the per-record counts between calls that differ in the window alone"""
    key = (id(items), k, lowercase_is_base, min_qual_char, data)
    per = None if counts_cache is None else counts_cache.get(key)
    if per is None:
        recs = records_of(data, min_qual_char)
        cat = b"".join(s + b"\n" for _, _, s, _ in recs)
        qcat = b"".join(q[:len(s)] + b"\n" for _, _, s, q in recs) if min_qual_char is not None else None
        holds, counts = _profile(cat, qcat, k, items, lowercase_is_base, min_qual_char)
        per, at = [], 0
        for _, _, s, _ in recs:
            m = max(0, len(s) - k + 1)
            per.append(counts[at:at + m][holds[at:at + m]])
            at += len(s) + 1
        if counts_cache is not None:
            counts_cache[key] = per
    out = np.zeros((len(per), 2), np.int64)
    for r, c in enumerate(per):
        out[r] = (len(c), ((c >= lower) & (c <= (np.iinfo(np.int64).max if upper is None else upper))).sum())
    return out


def _holds(h, n, bound, at_least):
    if isinstance(bound, float):
        ref, left = np.float64(bound) * n.astype(np.float64), h.astype(np.float64)
    else:
        ref, left = bound, h
    return left >= ref if at_least else left <= ref


def passes(nh: np.ndarray, min_hits=1, max_hits=None) -> np.ndarray:
    n, h = nh[:, 0], nh[:, 1]
    ok = (n >= 1) & _holds(h, n, min_hits, True)
    if max_hits is not None:
        ok &= _holds(h, n, max_hits, False)
    return ok


def filter_fastq(data1: bytes, k: int, items, data2: bytes = None, lower=1, upper=None, min_hits=1, max_hits=None, pair="any",
                 lowercase_is_base=True, min_qual_char=None, counts_cache=None) -> tuple:
    """(kept bytes of input 1, kept bytes of input 2 or None, totals: records, kept, passed, bases, kmers, hits)"""
    datas = [data1] if data2 is None else [data1, data2]
    assert pair in ("any", "both", "single") and not (pair == "single" and data2 is not None)
    recs = [records_of(d, min_qual_char) for d in datas]
    nhs = [read_hits(d, k, items, lower, upper, lowercase_is_base, min_qual_char, counts_cache) for d in datas]
    ok = [passes(nh, min_hits, max_hits) for nh in nhs]
    if data2 is not None:
        if len(recs[0]) != len(recs[1]):
            raise Malformed(min(len(recs[0]), len(recs[1])), "R1 and R2 differ in their number of records")
        keep = ok[0] | ok[1] if pair == "any" else ok[0] & ok[1]
        keeps = [keep, keep]
    elif pair == "single":
        keeps = ok
    else:
        if len(recs[0]) % 2:
            raise Malformed(len(recs[0]) - 1, "it has no mate: an odd number of records")
        p = ok[0].reshape(-1, 2)
        keeps = [np.repeat(p.any(1) if pair == "any" else p.all(1), 2)]
    outs = [b"".join(d[a:b] for (a, b, _, _), kp in zip(rs, keep) if kp) for d, rs, keep in zip(datas, recs, keeps)]
    totals = {"records": sum(len(r) for r in recs), "kept": int(sum(kp.sum() for kp in keeps)), "passed": int(sum(o.sum() for o in ok)),
              "bases": sum(len(s) for rs in recs for _, _, s, _ in rs), "kmers": int(sum(nh[:, 0].sum() for nh in nhs)),
              "hits": int(sum(nh[:, 1].sum() for nh in nhs))}
    return outs[0], outs[1] if data2 is not None else None, totals
