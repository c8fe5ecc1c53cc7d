#!/usr/bin/env python3
"""KmerTable.spectrum and KmerTable.query on the table of the bench workload (BASELINE config 2: 10 M pairs, k = 21, a mini table
sized as bench.py sizes it), timed with device events after warm-up:

  spectrum(10000)   one streaming pass over the slots, in its three forms (PG_SPECTRUM_BALLOT = 0: every count an LDS add; 1: the
                    lanes with c == 1 counted by a ballot, the default; 2: c == 2 as well), alternating, beside a plain device read of
                    the same bytes (torch's sum over the table, the "sum (R)" figure of tools/hbm_copy.py taken on this table);
  query             10^8 codes, half drawn from the table's own k-mers, half random 42-bit codes, shuffled.

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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=100_000_000)
    ap.add_argument("--high", type=int, default=10000)
    ap.add_argument("--load", type=float, default=0.6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "time_inspect.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k = 21
    cfg = synth.SynthConfig(n_pairs=a.pairs, n_barcodes=max(1, a.pairs // 200), read_len=150, seed=2022)
    s = synth.generate(cfg, device=dev, chunk_pairs=1 << 17, with_names=False)
    hint = max(1 << 14, int(1.05 * kmer.estimate_distinct(s, k)))
    table = kmer.KmerTable.alloc(k, dev, "mini", distinct_hint=hint, load=a.load).count(s)
    del s
    table.release_workspaces()
    res = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "k": k, "kind": table.kind, "log2_slots": table.log2_slots,
           "log2_bucket": table.log2_bucket, "table_bytes": table.nbytes, "occupancy": round(table.occupancy(), 4), "high": a.high}

    # ---- spectrum: the three ballot forms and the plain read, alternating (the rounds share whatever else the host is doing)
    lib = _lib.load()
    hist = torch.empty(a.high + 2, dtype=torch.int64, device=dev)
    words = table.data.view(torch.int32)
    stream = kmer._stream_ptr(dev)

    def spectrum():
        _lib.check(lib.pg_table_spectrum(table.desc(), a.high, hist.data_ptr(), stream))

    forms = {"ballot0": "0", "ballot1": "1", "ballot2": "2"}
    ms = {name: [] for name in list(forms) + ["plain_read"]}
    want = None
    for rnd in range(a.reps + 1):
        for name, env in forms.items():
            os.environ["PG_SPECTRUM_BALLOT"] = env
            got = timed(spectrum, a.warmup if rnd == 0 else 0, 1)
            h = hist.cpu()
            want = h if want is None else want
            assert torch.equal(h, want), f"{name}: another spectrum"
            if rnd:
                ms[name] += got
        got = timed(lambda: words.sum(), a.warmup if rnd == 0 else 0, 1)
        if rnd:
            ms["plain_read"] += got
    os.environ.pop("PG_SPECTRUM_BALLOT", None)
    res["spectrum"] = {name: dict(stats(v), read_TBps=round(table.nbytes / (sorted(v)[len(v) // 2] * 1e-3) / 1e12, 3)) for name, v in ms.items()}
    res["spectrum"]["time_over_plain_read"] = round(res["spectrum"]["ballot1"]["median_ms"] / res["spectrum"]["plain_read"]["median_ms"], 3)
    res["distinct_kmers"] = int(want.sum())
    res["share_with_count_1"] = round(float(want[1]) / max(1, int(want.sum())), 4)
    print(json.dumps(res["spectrum"]), flush=True)

    # ---- query
    n = a.queries
    own = table.compact()
    pick = (own[torch.randint(0, own.numel(), (n // 2,), device=dev)] >> _lib.HASH_COUNT_BITS) & ((1 << (2 * k)) - 1)     # (int64 slots: the shift is arithmetic)
    del own
    codes = torch.cat([pick, torch.randint(0, 1 << (2 * k), (n - n // 2,), device=dev, dtype=torch.int64)])
    del pick
    codes = codes[torch.randperm(n, device=dev)]
    counts = torch.empty(n, dtype=torch.int32, device=dev)

    def query():
        _lib.check(lib.pg_table_query(table.desc(), codes.data_ptr(), n, counts.data_ptr(), stream))

    q = timed(query, a.warmup, a.reps)
    found = int((counts > 0).sum())
    assert found >= n // 2 and int((counts < 0).sum()) == 0
    res["query"] = dict(stats(q), codes=n, found=found, Mcodes_per_s=round(n / (sorted(q)[len(q) // 2] * 1e-3) / 1e6, 1),
                        through_KmerTable_query_ms=stats(timed(lambda: table.query(codes), 1, 3))["median_ms"])
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
