"""A plain numpy / Python restatement of ``KmerTable.read_spans`` and ``KmerTable.trim_fastq`` (include/pangaea_feat.h, "Reads of a
FASTQ text trimmed to their solid span"), for the tests to compare with.  Nothing here is shared with the code under test; the
k-mer counts of a sequence line and the error type come from tests/_filter_ref.py.

  records    as in _filter_ref; in addition a quality line whose content (without a final ``\\r``) is shorter than the sequence
             line's (without its final ``\\r``) is malformed, with or without ``min_qual_char``
  solid      position i of the sequence line is solid iff it holds a k-mer whose count c has lower <= c <= upper
  run        a maximal interval [a, b) of solid positions; its span is (start a, length b - a + k - 1)
  first      the run with a = 0, else (0, 0)
  longest    the run with the largest b - a, the leftmost of equals, else (0, 0)
  trimmed    line 0, seq[start : start + length] + its line end, line 2, qual[start : start + length] + its line end
  passes     length >= min_len (None: k)
  pairs      any: both mates stay if either passes; both: if both pass; single: every record on its own
"""
import numpy as np

from ._filter_ref import Malformed, _profile


def records_of(data: bytes, min_qual_char=None) -> list:
    """[(line 0, sequence line, line 2, quality line, ends in a newline)] of every record, the lines without their ``\\n``;
    Malformed for the first bad record"""
    lines = data.split(b"\n")
    final_newline = lines[-1] == b"" and len(data) > 0
    if lines[-1] == b"":
        lines.pop()
    recs = []
    for r in range((len(lines) + 3) // 4):
        four = lines[4 * r:4 * r + 4]
        if len(four) < 4:
            raise Malformed(r, f"the text ends inside it ({len(four)} of 4 lines)")
        l0, l1, l2, l3 = four
        if l0[:1] != b"@":
            raise Malformed(r, "its first line does not begin with '@'")
        if l2[:1] != b"+":
            raise Malformed(r, "its third line does not begin with '+'")
        if min_qual_char is not None and len(l3) < len(l1):
            raise Malformed(r, "its quality line is shorter than its sequence line")
        if len(l3) - l3.endswith(b"\r") < len(l1) - l1.endswith(b"\r"):
            raise Malformed(r, "its quality line is shorter than its sequence line")
        recs.append((l0, l1, l2, l3, final_newline or 4 * r + 4 < len(lines)))
    return recs


def runs_of(solid: np.ndarray) -> list:
    """[(a, b)] of the maximal intervals [a, b) of True"""
    d = np.diff(np.concatenate([[0], np.asarray(solid, np.int8), [0]]))
    return list(zip(np.nonzero(d == 1)[0].tolist(), np.nonzero(d == -1)[0].tolist()))


def span_of(solid: np.ndarray, k: int, mode: str) -> tuple:
    """(start, length) of one record"""
    assert mode in ("first", "longest")
    runs = runs_of(solid)
    if mode == "first":
        runs = [r for r in runs if r[0] == 0]
    best = None
    for a, b in runs:
        if best is None or b - a > best[1] - best[0]:        # (strictly longer: the leftmost of equals stays)
            best = (a, b)
    return (0, 0) if best is None else (best[0], best[1] - best[0] + k - 1)


def profiles_of(data: bytes, k: int, items, lowercase_is_base=True, min_qual_char=None, cache=None) -> list:
    """[(holds, counts)] per record (``_filter_ref._profile``), the sequence lines looked at in one piece with a newline (no
    base) between them; ``cache`` (a dict) keeps them between calls that differ in window and mode alone"""
    key = (id(items), k, lowercase_is_base, min_qual_char, data)
    per = None if cache is None else cache.get(key)
    if per is None:
        recs = records_of(data, min_qual_char)
        cat = b"".join(s + b"\n" for _, s, _, _, _ in recs)
        qcat = b"".join(q[:len(s)] + b"\n" for _, s, _, q, _ in recs) if min_qual_char is not None else None
        holds, counts = _profile(cat, qcat, k, items, lowercase_is_base, min_qual_char)
        per, at = [], 0
        for _, s, _, _, _ in recs:
            m = max(0, len(s) - k + 1)
            per.append((holds[at:at + m], counts[at:at + m]))
            at += len(s) + 1
        if cache is not None:
            cache[key] = per
    return per


def solid_of(profile: tuple, lower=1, upper=None) -> np.ndarray:
    holds, counts = profile
    return holds & (counts >= lower) & (counts <= (np.iinfo(np.int64).max if upper is None else upper))


def read_spans(data: bytes, k: int, items, lower=1, upper=None, mode="longest", lowercase_is_base=True, min_qual_char=None,
               cache=None) -> np.ndarray:
    """int64 [n_records, 4]: (n, h, start, length) of every record"""
    per = profiles_of(data, k, items, lowercase_is_base, min_qual_char, cache)
    out = np.zeros((len(per), 4), np.int64)
    for r, p in enumerate(per):
        solid = solid_of(p, lower, upper)
        out[r] = (int(p[0].sum()), int(solid.sum())) + span_of(solid, k, mode)
    return out


def trimmed_record(rec: tuple, start: int, length: int) -> bytes:
    l0, l1, l2, l3, newline = rec
    cr_s, cr_q = l1.endswith(b"\r"), l3.endswith(b"\r")
    assert start + length <= len(l1) - cr_s
    return (l0 + b"\n" + l1[start:start + length] + (b"\r" if cr_s else b"") + b"\n" + l2 + b"\n" + l3[start:start + length]
            + (b"\r" if cr_q else b"") + (b"\n" if newline else b""))


def whole_record(rec: tuple) -> bytes:
    l0, l1, l2, l3, newline = rec
    return l0 + b"\n" + l1 + b"\n" + l2 + b"\n" + l3 + (b"\n" if newline else b"")


def trim_fastq(data1: bytes, k: int, items, data2: bytes = None, lower=1, upper=None, mode="longest", min_len=None, pair="both",
               lowercase_is_base=True, min_qual_char=None, cache=None) -> tuple:
    """(bytes written for input 1, for input 2 or None, totals: records, kept, passed, trimmed, bases, bases_out, kmers, hits)"""
    datas = [data1] if data2 is None else [data1, data2]
    assert pair in ("any", "both", "single") and not (pair == "single" and data2 is not None)
    min_len = k if min_len is None else min_len
    assert min_len >= 1
    recs = [records_of(d, min_qual_char) for d in datas]
    rows = [read_spans(d, k, items, lower, upper, mode, lowercase_is_base, min_qual_char, cache) for d in datas]
    ok = [row[:, 3] >= min_len for row in rows]
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
    outs, trimmed, bases_out = [], 0, 0
    for rs, row, keep in zip(recs, rows, keeps):
        parts = []
        for rec, (_, _, start, length), kp in zip(rs, row.tolist(), keep):
            if kp:
                parts.append(trimmed_record(rec, start, length))
                trimmed += len(parts[-1]) < len(whole_record(rec))
                bases_out += length
        outs.append(b"".join(parts))
    totals = {"records": sum(len(r) for r in recs), "kept": int(sum(kp.sum() for kp in keeps)), "passed": int(sum(o.sum() for o in ok)),
              "trimmed": int(trimmed), "bases": sum(len(r[1]) for rs in recs for r in rs), "bases_out": int(bases_out),
              "kmers": int(sum(row[:, 0].sum() for row in rows)), "hits": int(sum(row[:, 1].sum() for row in rows))}
    return outs[0], outs[1] if data2 is not None else None, totals
