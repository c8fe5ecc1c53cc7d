#!/usr/bin/env python3
"""Abundance rows against a finished table on the bench workload (BASELINE config 2: 10 M synthetic pairs, 50 k barcodes, k = 21, a
mini table of 2^16 buckets x 2^13 slots counted from those reads WITHOUT rows), timed after warm-up, several repeats, median / min /
max; (a) and (b) alternate inside one loop:

  (a) find     KmerTable.abundance_of end to end: the two scatter passes of the stream's records, pg_mini_find, the row shuffle
               (the partition plan is cached after the first call, as for a count of the same stream);
  (b) lookup   the same rows by pg_features, one random table line per k-mer occurrence (PG_MINI_FIND=0: the route before);
  (c) fused    count + rows of the same stream in one go (count(rows, emit) + features), for context;
  (d) copy     a plain device copy that moves the bytes (a) moves at least: the records written and read twice, the table read once.

--kernel-run: only a few calls of (a), for a kernel trace taken in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/time_find.py --kernel-run).

Prints one JSON document and writes it to --out.  Not a test: nothing here is a threshold."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pangaea_amd import kmer, synth  # noqa: E402
from tools.time_inspect import stats  # noqa: E402


def once(f) -> float:
    """milliseconds of one call of f between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--log2-slots", type=int, default=29)
    ap.add_argument("--log2-bucket", type=int, default=13)
    ap.add_argument("--min-len", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "time_find.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k, window, vsize = 21, 10, 400
    cfg = synth.SynthConfig(n_pairs=a.pairs, n_barcodes=max(1, a.pairs // 200), read_len=150, seed=2022)
    s = synth.generate(cfg, device=dev, chunk_pairs=1 << 17, with_names=False)
    rows = s.rows(a.min_len)
    plan = kmer.Plan(rows, dev)
    table = kmer.KmerTable.mini_with_slots(k, dev, a.log2_slots, a.log2_bucket).count(s)
    table.release_workspaces()
    abd_a = torch.empty((plan.n_rows, vsize), dtype=torch.int32, device=dev)
    abd_b = torch.empty_like(abd_a)

    def find():
        os.environ["PG_MINI_FIND"] = "1"
        table.abundance_of(s, plan, window, vsize, out=abd_a)

    def lookup():
        os.environ["PG_MINI_FIND"] = "0"
        table.abundance_of(s, plan, window, vsize, out=abd_b)

    if a.kernel_run:
        for _ in range(a.warmup + 3):
            find()
        torch.cuda.synchronize()
        assert table.rows_form == "find"
        return 0

    res = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "rows": plan.n_rows, "k": k, "window": window, "vsize": vsize,
           "log2_slots": table.log2_slots, "log2_bucket": table.log2_bucket, "table_bytes": table.nbytes, "entries": table._n_occupied()}
    fa, lb = [], []
    for i in range(a.warmup + a.reps):
        ta = once(find)
        assert table.rows_form == "find"
        tb = once(lookup)
        assert table.rows_form == "lookup"
        if i >= a.warmup:
            fa.append(ta)
            lb.append(tb)
    assert torch.equal(abd_a, abd_b), "the two forms disagree"
    n_records, n_long = table.plan_counts()
    med = lambda v: sorted(v)[len(v) // 2]
    res["records"] = n_records
    res["find"] = {"abundance_of": stats(fa)}
    res["lookup"] = {"abundance_of": stats(lb), "same_rows_as_find": True}
    res["find"]["over_lookup"] = round(med(fa) / med(lb), 3)
    res["find"]["faster_than_lookup_by_more_than_the_spread"] = bool(max(fa) < min(lb))
    print(json.dumps({"find": res["find"], "lookup": res["lookup"]}), flush=True)

    # ---- (c) the fused count + rows of the same stream
    fused = kmer.KmerTable.mini_with_slots(k, dev, a.log2_slots, a.log2_bucket)
    abd_c = torch.empty_like(abd_a)

    def count_and_rows():
        fused.reset().count(s, rows=plan, emit=(window, vsize))
        kmer.features(s, plan, k_tnf=None, table=fused, window=window, vsize=vsize, out_abd=abd_c)

    fc = []
    for i in range(a.warmup + a.reps):
        t = once(count_and_rows)
        if i >= a.warmup:
            fc.append(t)
    assert torch.equal(abd_c, abd_a), "the fused rows disagree"
    res["fused"] = {"count_and_rows": stats(fc), "same_rows_as_find": True}
    res["find"]["over_fused"] = round(med(fa) / med(fc), 3)
    del fused, abd_c

    # ---- (d) a copy of the bytes (a) moves: 12-byte records written and read by each scatter pass and read by the find kernel
    # (written twice, read twice -- the read of the stream and the words of the row shuffle are left out), the table read once
    moved = 4 * 12 * n_records + table.nbytes
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    cp = []
    for i in range(a.warmup + a.reps):
        t = once(lambda: dst.copy_(src))
        if i >= a.warmup:
            cp.append(t)
    res["bytes_moved"] = moved
    res["copy_of_bytes_moved"] = stats(cp)
    res["find"]["over_copy"] = round(med(fa) / med(cp), 3)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
