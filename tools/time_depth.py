#!/usr/bin/env python3
"""KmerTable.depth and KmerTable.profile on a 2 M-pair synth stream against its own k = 21 mini table, timed with device events
after 2 warm-up calls, 7 repeats, median [min - max]:

  depth (a)   every read as a range (4 * 10^6 ranges of 150 characters: the short form, nothing through memory)
  depth (b)   ranges of 50 000 characters tiling the stream (the long form, one workgroup per range selects)
  depth (c)   the whole stream as one range (what one very long range costs: one workgroup selects)
  profile     the whole stream

each beside what the library could do for the same answer before these entries: ``KmerTable.query`` on one 8-byte code per
position, prepared outside the timed region, then n_kmers / n_present / sum / max and a sort-based lower median in torch.  Both
answers are compared, both peak memories recorded (bytes allocated above what was held before the call).

Prints one JSON document and writes it to --out.  Not a test: nothing here is a threshold."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pangaea_amd import _lib, kmer, synth  # noqa: E402


def timed(f, warmup: int, reps: int) -> list:
    """milliseconds of ``reps`` calls of f, each between two device events, after ``warmup`` calls"""
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ms: list) -> dict:
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "reps": len(s)}


def peak_of(f) -> tuple:
    """(result of f, bytes it allocated above what was held when it was called)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    out = f()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - held


def codes_of(s, k: int) -> torch.Tensor:
    """int64 [n_chars]: the forward code of the k-mer that starts at every position (first character highest), -1 where none does
    -- the input ``KmerTable.query`` wants, built with torch from the stream's words"""
    dev, n = s.codes.device, s.n_chars
    sh = torch.arange(32, device=dev)
    chars = ((s.codes[:, None] >> (2 * sh)[None, :]) & 3).reshape(-1)[:n]
    bad = (((s.lenient_valid()[:, None] >> sh[None, :]) & 1) == 0).reshape(-1)[:n]
    before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(bad, 0)])
    del bad
    m = n - k + 1
    code = torch.zeros(m, dtype=torch.int64, device=dev)
    for j in range(k):
        code = (code << 2) | chars[j:j + m]
    code[(before[k:] - before[:m]) != 0] = -1
    return torch.cat([code, torch.full((k - 1,), -1, dtype=torch.int64, device=dev)])


def composed(table, codes: torch.Tensor, starts: torch.Tensor, length: int, k: int) -> torch.Tensor:
    """the five numbers of every range [start, start + length) from query + torch: a sort per range for the lower median"""
    q = table.query(codes)                                                     # int64, -1 where no k-mer starts
    pos = starts[:, None] + torch.arange(length - k + 1, device=codes.device)[None, :]
    v = q[pos]
    del pos, q
    have = v >= 0
    n = have.sum(1)
    v0 = torch.where(have, v, 0)
    out = torch.stack([n, (v0 > 0).sum(1), v0.sum(1), v0.max(1).values], 1)
    del v0
    ordered = torch.sort(torch.where(have, v, 1 << 40), 1).values              # what holds no k-mer goes last
    med = ordered.gather(1, ((n - 1) // 2).clamp(min=0)[:, None])[:, 0]
    return torch.cat([out, torch.where(n > 0, med, 0)[:, None]], 1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--load", type=float, default=0.6)
    ap.add_argument("--tile", type=int, default=50_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "time_depth.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k = 21
    cfg = synth.SynthConfig(n_pairs=a.pairs, n_barcodes=max(1, a.pairs // 200), read_len=150, seed=2022)
    s = synth.generate(cfg, device=dev, chunk_pairs=1 << 17, with_names=False)
    hint = max(1 << 14, int(1.05 * kmer.estimate_distinct(s, k)))
    table = kmer.KmerTable.alloc(k, dev, "mini", distinct_hint=hint, load=a.load).count(s)
    table.release_workspaces()
    n = s.n_chars
    res = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "k": k, "kind": table.kind, "log2_slots": table.log2_slots,
           "log2_bucket": table.log2_bucket, "table_bytes": table.nbytes, "n_chars": n, "short_max": _lib.DEPTH_SHORT_MAX,
           "warmup": a.warmup, "reps": a.reps}
    codes = codes_of(s, k)
    p = torch.arange(a.pairs, device=dev, dtype=torch.int64) * 302
    shapes = {"a_every_read": (torch.stack([p, p + 151], 1).reshape(-1), 150),
              "b_tiles": (torch.arange(n // a.tile, device=dev, dtype=torch.int64) * a.tile, a.tile),
              "c_whole_stream": (torch.zeros(1, dtype=torch.int64, device=dev), n)}
    for name, (starts, length) in shapes.items():
        ends = starts + length
        got, peak_new = peak_of(lambda: table.depth(s, (starts, ends)))
        want, peak_old = peak_of(lambda: composed(table, codes, starts, length, k))
        assert torch.equal(got, want), f"{name}: the two answers differ"
        del want
        new = timed(lambda: table.depth(s, (starts, ends)), a.warmup, a.reps)
        old = timed(lambda: composed(table, codes, starts, length, k), a.warmup, a.reps)
        res[name] = {"ranges": int(starts.numel()), "characters_each": length, "depth": dict(stats(new), peak_bytes=peak_new),
                     "query_and_torch": dict(stats(old), peak_bytes=peak_old, codes_bytes=codes.numel() * 8),
                     "speedup": round(sorted(old)[len(old) // 2] / sorted(new)[len(new) // 2], 2),
                     "median_of_medians": int(got[:, _lib.DEPTH_MEDIAN].median())}
        print(name, json.dumps(res[name]), flush=True)
        table.release_workspaces()
    got, peak_new = peak_of(lambda: table.profile(s))
    want, peak_old = peak_of(lambda: table.query(codes))
    assert torch.equal(got, want), "profile and query differ"
    del got, want
    new = timed(lambda: table.profile(s), a.warmup, a.reps)
    old = timed(lambda: table.query(codes), a.warmup, a.reps)
    res["profile"] = {"positions": n, "profile": dict(stats(new), peak_bytes=peak_new),
                      "query": dict(stats(old), peak_bytes=peak_old, codes_bytes=codes.numel() * 8),
                      "speedup": round(sorted(old)[len(old) // 2] / sorted(new)[len(new) // 2], 2)}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
