"""A plain numpy / Python restatement of ``KmerTable.read_depths`` and ``KmerTable.normalize_fastq`` (include/pangaea_feat.h, "Depth of
the reads of a FASTQ text"), for the tests to compare with.  Records and k-mers are those of tests/_filter_ref.py; nothing here
is shared with the code under test.

  value      of a k-mer: its count c in the table (0: absent), taken as 0 when c < lower
  row        n = the record's k-mers, present = its values > 0, d = sorted(values)[((n - 1) * percentile) // 100], 0 when n = 0
  draw       of unit u, in Python integers reduced mod 2^64 by hand (``draw`` below): 24 bits
  unit       record r of its file is unit r >> 1 for mates interleaved in one file, unit r otherwise (R1 / R2: record i of both
             files is unit i; single: every record is its own)
  passes     n >= 1 and d >= min_depth and w * d < target * 2^24, in exact integers
  pairs      any: both mates stay if either passes; both: if both pass; single: every record on its own
"""
import numpy as np

from ._filter_ref import Malformed, kmer_counts, records_of  # noqa: F401  (Malformed: what the tests catch)

M64 = (1 << 64) - 1


def draw(seed: int, unit: int) -> int:
    z = (seed + (unit + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 40


def record_counts(data: bytes, k: int, items, lowercase_is_base=True, min_qual_char=None, cache=None) -> list:
    """the table's counts of every record's k-mers, in order: a list of int64 arrays.  ``cache`` (a dict) keeps them between calls
    that differ in lower, percentile and the rule alone (``read_depths`` keeps its rows there too)"""
    key = (id(items), k, lowercase_is_base, min_qual_char, data)
    if cache is not None and key in cache:
        return cache[key]
    per = [kmer_counts(s, q, k, items, lowercase_is_base, min_qual_char) for _, _, s, q in records_of(data, min_qual_char)]
    if cache is not None:
        cache[key] = per
    return per


def read_depths(data: bytes, k: int, items, lower=1, percentile=50, lowercase_is_base=True, min_qual_char=None, cache=None) -> np.ndarray:
    """int64 [n_records, 3]: (n, present, d) of every record"""
    assert lower >= 1 and 0 <= percentile <= 100
    key = ("rows", id(items), k, lower, percentile, lowercase_is_base, min_qual_char, data)
    if cache is not None and key in cache:
        return cache[key]
    per = record_counts(data, k, items, lowercase_is_base, min_qual_char, cache)
    out = np.zeros((len(per), 3), np.int64)
    for r, c in enumerate(per):
        v = sorted(int(x) if x >= lower else 0 for x in c)
        n = len(v)
        out[r] = (n, sum(1 for x in v if x > 0), v[((n - 1) * percentile) // 100] if n else 0)
    out.setflags(write=False)
    if cache is not None:
        cache[key] = out
    return out


def passes(rows: np.ndarray, w: list, target: int, min_depth: int) -> tuple:
    """(passes, low) per record, from Python integers"""
    low = [int(n) < 1 or int(d) < min_depth for n, _, d in rows]
    ok = [not lo and wi * int(d) < target << 24 for lo, wi, (_, _, d) in zip(low, w, rows)]
    return np.array(ok, bool), np.array(low, bool)


def normalize_fastq(data1: bytes, k: int, items, data2: bytes = None, target=None, min_depth=0, lower=1, percentile=50, pair="any", seed=0,
                    lowercase_is_base=True, min_qual_char=None, cache=None) -> tuple:
    """(kept bytes of input 1, kept bytes of input 2 or None, totals: records, kept, passed, low, bases, kmers, hits, depth_in,
    depth_out)"""
    datas = [data1] if data2 is None else [data1, data2]
    assert pair in ("any", "both", "single") and not (pair == "single" and data2 is not None)
    assert 1 <= target < 1 << 31 and min_depth >= 0 and 0 <= seed <= M64
    recs = [records_of(d, min_qual_char) for d in datas]
    rows = [read_depths(d, k, items, lower, percentile, lowercase_is_base, min_qual_char, cache) for d in datas]
    shift = 1 if data2 is None and pair != "single" else 0
    judged = [passes(rw, [draw(seed, r >> shift) for r in range(len(rw))], target, min_depth) for rw in rows]
    ok, low = [j[0] for j in judged], [j[1] for j in judged]
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
              "low": int(sum(lo.sum() for lo in low)), "bases": sum(len(s) for rs in recs for _, _, s, _ in rs),
              "kmers": int(sum(rw[:, 0].sum() for rw in rows)), "hits": int(sum(rw[:, 1].sum() for rw in rows)),
              "depth_in": int(sum(rw[:, 2].sum() for rw in rows)), "depth_out": int(sum(rw[kp, 2].sum() for rw, kp in zip(rows, keeps)))}
    return outs[0], outs[1] if data2 is not None else None, totals
