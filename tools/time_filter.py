#!/usr/bin/env python3
"""KmerTable.filter_fastq on the bench table: a synth stream of --pairs read pairs (bench.py's configuration: k = 21, mini table,
load 0.6) is counted, its first --fastq-pairs pairs are written as interleaved FASTQ (synth.write_fastq_fast), and on that text

  index    pg_fastq_index      (newline counts, their scan, the line starts)
  hits     pg_table_read_hits  (one wavefront per record: (k-mers, hits) from the ASCII text)
  gather   pg_fastq_gather     (the records with h >= n / 2, to their places)

are timed with device events after --warmup calls, --reps repeats, median [min - max]; then the whole call, file to file
(wall seconds and the device_ms it reports).  Two reference times from the same run stand beside them:

  (a) copy     a device-to-device copy of the same text bytes (tools/hbm_copy.py's method)
  (b) profile  KmerTable.profile over the packed stream of the same reads: the kernel that already does the same lookups, one per
               position, and writes 4 bytes for each (pg_table_profile itself, as the three above are entries; the Python method,
               which widens the answers to int64, is recorded beside it as ``profile_method``)

``hits_over_profile`` is the ratio of the medians, ``profile_spread`` (b)'s own (max - min) / median over its repeats: the hits
kernel does (b)'s lookups and writes far less, so the expectation is a ratio of at most 1 + spread.  Nothing here is a threshold.

Prints one JSON document and writes it to --out."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pangaea_amd import _lib, fastqtext, kmer, synth  # noqa: E402
from pangaea_amd.kmer import _stream_ptr  # noqa: E402


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
    ap.add_argument("--pairs", type=int, default=10_000_000, help="pairs the table is counted from (bench.py: 10 M)")
    ap.add_argument("--fastq-pairs", type=int, default=1_000_000, help="pairs written as FASTQ and filtered (692 bytes each)")
    ap.add_argument("--load", type=float, default=0.6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "time_filter.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k = 21
    L = _lib.load()
    cfg = synth.SynthConfig(n_pairs=a.pairs, n_barcodes=max(1, a.pairs // 200), read_len=150, seed=2022)
    s = synth.generate(cfg, device=dev, chunk_pairs=1 << 17, with_names=False)
    hint = max(1 << 14, int(1.05 * kmer.estimate_distinct(s, k)))
    table = kmer.KmerTable.alloc(k, dev, "mini", distinct_hint=hint, load=a.load).count(s)
    table.release_workspaces()
    n_fq = min(a.fastq_pairs, a.pairs)
    res = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "fastq_pairs": n_fq, "k": k, "kind": table.kind, "log2_slots": table.log2_slots,
           "log2_bucket": table.log2_bucket, "table_bytes": table.nbytes, "warmup": a.warmup, "reps": a.reps,
           "piece_bytes": fastqtext.piece_bytes()}
    with tempfile.TemporaryDirectory() as tmp:
        fq, out = os.path.join(tmp, "reads.fq"), os.path.join(tmp, "kept.fq")
        synth.write_fastq_fast(s, cfg, fq, n_fq)
        data = np.fromfile(fq, dtype=np.uint8)
        n = int(data.size)
        text = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        text[:n] = torch.from_numpy(data).to(dev)
        del data
        res["text_bytes"] = n
        sp = _stream_ptr(dev)
        # the three kernels, entry by entry
        idx, n_lines = fastqtext.line_index(text, n)
        n_rec = n_lines // 4
        assert n_lines == 8 * n_fq
        ws = torch.empty(L.pg_fastq_index_workspace_bytes(n), dtype=torch.uint8, device=dev)
        word = torch.zeros(1, dtype=torch.int64, device=dev)
        res["index"] = stats(timed(lambda: _lib.check(L.pg_fastq_index(text.data_ptr(), n, idx.data_ptr(), idx.numel(), word.data_ptr(), ws.data_ptr(),
                                                                        ws.numel(), sp)), a.warmup, a.reps))
        hits = torch.empty((n_rec, 2), dtype=torch.int32, device=dev)
        status = torch.zeros(2, dtype=torch.int64, device=dev)
        hits_ms = timed(lambda: _lib.check(L.pg_table_read_hits(table.desc(), k, text.data_ptr(), n, idx.data_ptr(), n_rec, 0, 1, -1, 1, 0, hits.data_ptr(),
                                                                status.data_ptr(), sp)), a.warmup, a.reps)
        res["hits"] = stats(hits_ms)
        assert status.tolist() == [0, -1]
        keep = (hits[:, 0] >= 1) & (2 * hits[:, 1] >= hits[:, 0])
        kept = keep.nonzero().flatten()
        lens = idx[4 * kept + 4] - idx[4 * kept]
        dst = torch.cumsum(lens, 0) - lens
        total = int(lens.sum())
        outbuf = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        res["gather"] = dict(stats(timed(lambda: _lib.check(L.pg_fastq_gather(text.data_ptr(), n, idx.data_ptr(), n_rec, kept.data_ptr(), dst.data_ptr(),
                                                                              int(kept.numel()), outbuf.data_ptr(), outbuf.numel(), sp)), a.warmup, a.reps)),
                             kept_records=int(kept.numel()), kept_bytes=total)
        res["kmers"], res["hits_total"] = int(hits[:, 0].sum()), int(hits[:, 1].sum())
        # (a) the same bytes copied device to device
        other = torch.empty_like(text)
        res["copy"] = stats(timed(lambda: other.copy_(text), a.warmup, a.reps))
        del other, outbuf
        # (b) the parent's profile over the packed stream of the same reads
        n_chars = 302 * n_fq
        plane = s.lenient_valid().contiguous()
        counts = torch.empty(n_chars, dtype=torch.int32, device=dev)
        prof_ms = timed(lambda: _lib.check(L.pg_table_profile(table.desc(), s.codes.data_ptr(), plane.data_ptr(), s.n_chars, 0, n_chars, counts.data_ptr(), sp)),
                        a.warmup, a.reps)
        res["profile"] = dict(stats(prof_ms), positions=n_chars)
        del counts
        # (... and through its Python method, which widens the 4-byte answers to int64)
        res["profile_method"] = stats(timed(lambda: table.profile(s, 0, n_chars), a.warmup, a.reps))
        med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
        res["hits_over_profile"] = round(med(hits_ms) / med(prof_ms), 3)
        res["profile_spread"] = round((max(prof_ms) - min(prof_ms)) / med(prof_ms), 3)
        del text, idx
        # the whole call, file to file (the page cache holds the file: it was written a moment ago)
        calls = []
        for _ in range(a.warmup + a.reps):
            calls.append(table.filter_fastq(fq, out, min_hits=0.5, pair="any"))
        calls = calls[a.warmup:]
        res["whole_call"] = {"seconds": stats([1000 * c["seconds"] for c in calls]), "device_ms": stats([c["device_ms"] for c in calls]),
                             "totals": {n_: calls[-1][n_] for n_ in ("records", "kept", "passed", "bases", "kmers", "hits")},
                             "out_bytes": os.path.getsize(out)}
        res["whole_call"]["seconds"] = {n_.replace("_ms", "_s"): round(v / 1000, 4) if n_ != "reps" else v for n_, v in res["whole_call"]["seconds"].items()}
    text_out = json.dumps(res, indent=1)
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text_out + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
