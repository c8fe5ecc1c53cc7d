"""A plain numpy / Python restatement of ``KmerTable.read_corrections`` and ``KmerTable.correct_fastq`` (include/pangaea_feat.h,
"Single substitutions in the reads of a FASTQ text put right"), for the tests to compare with.  Nothing here is shared with the
code under test; the k-mer counts of a sequence line come from tests/_filter_ref.py, the records from tests/_trim_ref.py.

  bases      of a sequence line: its bytes without a final ``\\r``; len of them, n_pos = max(0, len - k + 1)
  classes    position i < n_pos is S (it holds a k-mer whose count c has lower <= c <= upper), W (it holds a k-mer whose count has
             not) or V (it holds none); positions -1 and n_pos are E
  candidate  a maximal run [a, b) of W whose neighbours are both in {S, E}, not both E, and
                 S .. S with b - a == k:  p = b - 1          E .. S with b - a <= k:  p = b - 1
                 S .. E with b - a <= k:  p = a + k - 1
  valid      a base x other than the one at p (without regard to case) such that all b - a k-mers at [a, b), read with x at p,
             have a count inside the window
  corrected  exactly one valid x: byte p becomes x in the letter case it had; everything else stays
  one pass   every candidate is judged on the record as it came
"""
import numpy as np

from ._filter_ref import Malformed, _profile  # noqa: F401  (Malformed: what records_of raises)
from ._trim_ref import records_of

S, W, V, E = "S", "W", "V", "E"


def bases_of(line: bytes) -> bytes:
    return line[:-1] if line.endswith(b"\r") else line


def profiles_of(data: bytes, k: int, items, lowercase_is_base=True, min_qual_char=None, cache=None) -> list:
    """[(holds, counts)] per record over the bases of its sequence line, the lines looked at in one piece with a newline (no
    base) between them; ``cache`` (a dict) keeps them between calls that differ in the window alone"""
    key = (id(items), k, lowercase_is_base, min_qual_char, data)
    per = None if cache is None else cache.get(key)
    if per is None:
        recs = records_of(data, min_qual_char)
        seqs = [bases_of(r[1]) for r in recs]
        cat = b"".join(s + b"\n" for s in seqs)
        qcat = b"".join(r[3][:len(s)] + b"\n" for r, s in zip(recs, seqs)) if min_qual_char is not None else None
        holds, counts = _profile(cat, qcat, k, items, lowercase_is_base, min_qual_char)
        per, at = [], 0
        for s in seqs:
            m = max(0, len(s) - k + 1)
            per.append((holds[at:at + m], counts[at:at + m]))
            at += len(s) + 1
        if cache is not None:
            cache[key] = per
    return per


def _inside(counts, lower, upper):
    return (counts >= lower) & (counts <= (np.iinfo(np.int64).max if upper is None else upper))


def classes_of(profile: tuple, lower=1, upper=None) -> str:
    """one letter of S, W, V per position"""
    holds, counts = profile
    ok = _inside(counts, lower, upper)
    return "".join(V if not h else S if o else W for h, o in zip(holds.tolist(), ok.tolist()))


def candidates_of(classes: str, k: int) -> list:
    """[(a, b, p)] of one record's candidates, in order"""
    n_pos = len(classes)
    out, i = [], 0
    while i < n_pos:
        if classes[i] != W:
            i += 1
            continue
        a = i
        while i < n_pos and classes[i] == W:
            i += 1
        b = i
        left = E if a == 0 else classes[a - 1]
        right = E if b == n_pos else classes[b]
        if left == V or right == V or (left == E and right == E):
            continue
        if left == S and right == S:
            if b - a == k:
                out.append((a, b, b - 1))
        elif b - a <= k:
            out.append((a, b, b - 1 if right == S else a + k - 1))
    return out


def valid_bases(seq: bytes, qual, a: int, b: int, p: int, k: int, items, lower=1, upper=None, lowercase_is_base=True,
                min_qual_char=None) -> list:
    """the upper-case bases x that make all k-mers at [a, b) solid when they stand at p"""
    out = []
    for x in b"ACGT":
        if x == seq[p] or (lowercase_is_base and x == (seq[p] & 0xDF)):
            continue
        alt = seq[a:p] + bytes([x]) + seq[p + 1:b + k - 1]
        holds, counts = _profile(alt, None if qual is None else qual[a:b + k - 1], k, items, lowercase_is_base, min_qual_char)
        assert len(holds) == b - a and holds.all()
        if _inside(counts, lower, upper).all():
            out.append(x)
    return out


def correct_record(seq: bytes, qual, profile: tuple, k: int, items, lower=1, upper=None, lowercase_is_base=True, min_qual_char=None) -> tuple:
    """((n, h, candidates, corrected), the corrected bases, [(a, b, p, valid bases)]) of one record; ``seq``: the bases of its
    sequence line, ``qual``: its quality line (looked at under ``min_qual_char`` only)"""
    cls = classes_of(profile, lower, upper)
    fixed = bytearray(seq)
    detail = []
    for a, b, p in candidates_of(cls, k):
        valid = valid_bases(seq, qual if min_qual_char is not None else None, a, b, p, k, items, lower, upper, lowercase_is_base, min_qual_char)
        detail.append((a, b, p, valid))
        if len(valid) == 1:
            fixed[p] = valid[0] | (seq[p] & 0x20)
    corrected = sum(len(d[3]) == 1 for d in detail)
    return (len(cls) - cls.count(V), cls.count(S), len(detail), corrected), bytes(fixed), detail


def read_corrections(data: bytes, k: int, items, lower=1, upper=None, lowercase_is_base=True, min_qual_char=None, cache=None) -> tuple:
    """(rows: int64 [n_records, 4] -- n, h, candidates, corrected --, the corrected text, gained: the sum of b - a over the corrected
    runs per record, details per record)"""
    recs = records_of(data, min_qual_char)
    per = profiles_of(data, k, items, lowercase_is_base, min_qual_char, cache)
    rows = np.zeros((len(recs), 4), np.int64)
    gained = np.zeros(len(recs), np.int64)
    parts, details = [], []
    for r, ((l0, l1, l2, l3, newline), prof) in enumerate(zip(recs, per)):
        seq = bases_of(l1)
        row, fixed, detail = correct_record(seq, l3, prof, k, items, lower, upper, lowercase_is_base, min_qual_char)
        rows[r] = row
        gained[r] = sum(b - a for a, b, _, valid in detail if len(valid) == 1)
        details.append(detail)
        parts.append(l0 + b"\n" + fixed + l1[len(seq):] + b"\n" + l2 + b"\n" + l3 + (b"\n" if newline else b""))
    out = b"".join(parts)
    assert len(out) == len(data)
    return rows, out, gained, details


def correct_fastq(data1: bytes, k: int, items, data2: bytes = None, lower=1, upper=None, lowercase_is_base=True, min_qual_char=None,
                  cache=None) -> tuple:
    """(bytes written for input 1, for input 2 or None, totals: records, bases, kmers, hits, candidates, corrected,
    reads_corrected)"""
    datas = [data1] if data2 is None else [data1, data2]
    got = [read_corrections(d, k, items, lower, upper, lowercase_is_base, min_qual_char, cache) for d in datas]
    if data2 is not None and len(got[0][0]) != len(got[1][0]):
        raise Malformed(min(len(got[0][0]), len(got[1][0])), "R1 and R2 differ in their number of records")
    rows = np.concatenate([g[0] for g in got])
    totals = {"records": int(len(rows)), "bases": sum(len(r[1]) for d in datas for r in records_of(d, min_qual_char)),
              "kmers": int(rows[:, 0].sum()), "hits": int(rows[:, 1].sum()), "candidates": int(rows[:, 2].sum()),
              "corrected": int(rows[:, 3].sum()), "reads_corrected": int((rows[:, 3] > 0).sum())}
    return got[0][1], got[1][1] if data2 is not None else None, totals
