#!/usr/bin/env python3
"""sortreads.sort_fastq on a pair-shuffled synthetic file: N_PAIRS read pairs (bench.py's data: 150-base reads, 200 pairs per
barcode, 2 % untagged) are written as interleaved 10x-style FASTQ (synth.write_fastq_fast), shuffled at pair level with a fixed
seed on the device, and on that text

  index    pg_fastq_index          (the line starts)
  tags     pg_fastq_barcode_tags   (one wavefront per header)
  sort     pg_fastq_tag_keys + torch.sort(stable), one pass per 8-byte chunk of the longest tag, and the class pass
  compare  pg_fastq_tag_compare    (on the final order: the check every sort runs)
  gather   pg_fastq_gather         (the records to their places, in the sorted order)

are timed entry by entry with device events after --warmup calls, --reps repeats, median [min - max]; then the whole call, file to
file (wall seconds and the per-stage device_ms it reports).  Two device copies from the same run stand beside them:

  copy_text     the text's bytes, device to device: what the gather is compared with
  copy_headers  as many bytes as the headers the tags kernel reads

``gather_bytes_per_ms`` is to be read beside profiles/time_filter.json (gather: kept_bytes / median_ms, records in input order
there, in sorted order here); ``tags_over_copy_headers`` is the ratio of the medians.  --host-baseline adds the wall time of
``LC_ALL=C sort -s -k1,1`` on a one-line-per-pair, tag-prefixed form of the same data (written by this tool; the time to write it
is not counted).  Nothing here is a threshold.

Prints one JSON document and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pangaea_amd import _lib, fastqtext, sortreads, synth  # noqa: E402


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


def host_baseline(fq: str, tmp: str) -> dict:
    """wall seconds of ``LC_ALL=C sort -s -k1,1`` on one line per pair: the tag (``~~~`` without one), a tab, the pair's eight lines
    joined by tabs"""
    import re
    tag = re.compile(rb"BX:Z:[^ \t\n\v\f\r]+")
    flat, out = os.path.join(tmp, "flat.txt"), os.path.join(tmp, "flat.sorted.txt")
    with open(fq, "rb") as src, open(flat, "wb") as dst:
        while True:
            block = [src.readline() for _ in range(8)]
            if not block[0]:
                break
            m = tag.search(block[0])
            dst.write((m.group(0) if m else b"~~~") + b"\t" + b"\t".join(x.rstrip(b"\n") for x in block) + b"\n")
    t0 = time.perf_counter()
    subprocess.run(["sort", "-s", "-k1,1", "-o", out, flat], check=True, env=dict(os.environ, LC_ALL="C"))
    return {"seconds": round(time.perf_counter() - t0, 3), "bytes": os.path.getsize(flat), "command": "LC_ALL=C sort -s -k1,1"}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", nargs="?", type=int, default=10_000_000, help="read pairs (bench.py: 10 M, 6.9 GB of text)")
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "time_sort.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.load()
    cfg = synth.SynthConfig(n_pairs=a.pairs, n_barcodes=max(1, a.pairs // 200), read_len=150, seed=a.seed)
    res = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "seed": a.seed, "warmup": a.warmup, "reps": a.reps,
           "piece_bytes": fastqtext.piece_bytes()}
    with tempfile.TemporaryDirectory() as tmp:
        made, fq, out = os.path.join(tmp, "made.fq"), os.path.join(tmp, "shuffled.fq"), os.path.join(tmp, "sorted.fq")
        s = synth.generate(cfg, device=dev, chunk_pairs=1 << 17, with_names=False)
        synth.write_fastq_fast(s, cfg, made)
        del s
        # the pairs in a random order (a fixed seed), made on the device with the gather itself
        text, n = sortreads._read_text(made, dev)
        os.remove(made)
        idx, n_lines = sortreads.line_index(text, n)
        assert n_lines == 8 * a.pairs
        gen = torch.Generator(device="cpu").manual_seed(a.seed)
        shuffle = torch.randperm(a.pairs, generator=gen).to(dev)
        mixed = torch.empty(n + 32, dtype=torch.uint8, device=dev)
        sortreads._gather_run(sortreads._gather_plan([text], [n], [idx], shuffle), mixed, n)
        with open(fq, "wb") as f:
            step = 1 << 28
            for at in range(0, n, step):
                f.write(memoryview(mixed[at:min(n, at + step)].cpu().numpy()))
        del text, idx, shuffle
        text = mixed
        res["text_bytes"] = n
        # entry by entry
        ws = torch.empty(L.pg_fastq_index_workspace_bytes(n), dtype=torch.uint8, device=dev)
        idx, n_lines = sortreads.line_index(text, n)
        word = torch.zeros(1, dtype=torch.int64, device=dev)
        sp = sortreads._stream_ptr(dev)
        res["index"] = stats(timed(lambda: _lib.check(L.pg_fastq_index(text.data_ptr(), n, idx.data_ptr(), idx.numel(), word.data_ptr(), ws.data_ptr(),
                                                                        ws.numel(), sp)), a.warmup, a.reps))
        del ws
        tags_ms = timed(lambda: sortreads.barcode_tags(text, idx, a.pairs, 8, n), a.warmup, a.reps)
        off, length, status = sortreads.barcode_tags(text, idx, a.pairs, 8, n)
        assert status.tolist() == [0, -1]
        header_bytes = int((idx[1:8 * a.pairs:8] - idx[0:8 * a.pairs:8]).sum())
        longest = int(length.max()) - 5
        res["tags"] = dict(stats(tags_ms), header_bytes=header_bytes, untagged=int((length == 0).sum()), longest_tag=longest)
        sort_ms = timed(lambda: sortreads._order_of(text, n, off, length, longest), a.warmup, a.reps)
        order, passes = sortreads._order_of(text, n, off, length, longest)
        res["sort"] = dict(stats(sort_ms), passes=passes)
        keys_ms = timed(lambda: sortreads.tag_keys(text, off, length, order, 0, n), a.warmup, a.reps)
        res["sort"]["keys_one_pass"] = stats(keys_ms)
        cmp_ms = timed(lambda: sortreads.tag_compare(text, off, length, order, n), a.warmup, a.reps)
        cmp_sorted = sortreads.tag_compare(text, off, length, order, n)
        assert not bool((cmp_sorted == 1).any())
        res["compare"] = dict(stats(cmp_ms), runs=int((cmp_sorted == -1).sum()) + 1)
        out_dev = torch.empty(n + 32, dtype=torch.uint8, device=dev)
        plan = sortreads._gather_plan([text], [n], [idx], order)
        gather_ms = timed(lambda: sortreads._gather_run(plan, out_dev, n), a.warmup, a.reps)
        res["gather"] = dict(stats(gather_ms), records=2 * a.pairs, bytes=n)
        res["gather_plan"] = stats(timed(lambda: sortreads._gather_plan([text], [n], [idx], order), a.warmup, a.reps))
        del plan
        # the two copies
        copy_ms = timed(lambda: out_dev[:n].copy_(text[:n]), a.warmup, a.reps)
        res["copy_text"] = stats(copy_ms)
        head_ms = timed(lambda: out_dev[:header_bytes].copy_(text[:header_bytes]), a.warmup, a.reps)
        res["copy_headers"] = stats(head_ms)
        med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
        res["gather_bytes_per_ms"] = round(n / med(gather_ms))
        res["copy_text_bytes_per_ms"] = round(n / med(copy_ms))
        res["gather_over_copy_text"] = round(med(gather_ms) / med(copy_ms), 3)
        res["tags_over_copy_headers"] = round(med(tags_ms) / med(head_ms), 3)
        del text, mixed, idx, out_dev, off, length, order, cmp_sorted
        torch.cuda.empty_cache()
        # the whole call, file to file (the page cache holds the file: it was written a moment ago)
        calls = [sortreads.sort_fastq(fq, out) for _ in range(a.warmup + a.reps)][a.warmup:]
        res["whole_call"] = {"seconds": {k.replace("_ms", "_s"): v for k, v in stats([c["seconds"] for c in calls]).items()},
                             "device_ms": {stage: stats([c["device_ms"][stage] for c in calls]) for stage in sortreads.STAGES},
                             "result": {k: calls[-1][k] for k in ("pairs", "barcodes", "untagged_pairs", "longest_tag", "passes", "already_sorted", "bytes")}}
        check = sortreads.check_fastq(out)
        assert check["sorted"] and check["pairs"] == a.pairs
        if a.host_baseline:
            res["host_baseline"] = host_baseline(fq, tmp)
    text_out = json.dumps(res, indent=1)
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text_out + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
