#!/usr/bin/env python3
"""KmerTable.correct_fastq on the bench table: tools/time_trim.py's table and text -- a synth stream of --pairs read pairs (bench.py's
configuration: k = 21, mini table, load 0.6) is counted, its first --fastq-pairs pairs are written as interleaved FASTQ
(synth.write_fastq_fast) -- and on that text, under the count window [--lower, none] (2: k-mers seen once are the errors'),

  correct_rows      pg_table_correct_reads, out = NULL      (one wavefront per record: n, h, candidates, corrected; nothing stored)
  correct_out       pg_table_correct_reads, out = a copy    (... and the corrected bytes into a buffer that holds the text)
  correct_in_place  pg_table_correct_reads, out = text      (... into the text itself, which is restored before every call,
                                                             outside the timed events)

are timed with device events after --warmup calls, --reps repeats, median [min - max]; then the whole call, file to file (wall
seconds and the device_ms it reports).  Two reference times from the same run stand beside them:

  spans             pg_table_read_spans (PG_SPAN_LONGEST) on the same text and window: the kernel that already does the same
                    staging, lookups and run walk, and that this tool's subject does not touch
  copy              a device copy of the same bytes

``correct_over_spans`` are the ratios of the medians, ``spans_spread`` the spans kernel's own (max - min) / median over its
repeats.  The expectation: the run walk costs what SpanRuns costs, the rest is proportional to the candidates per read (one text
read of at most 61 lanes and three lookups per lane each).  Nothing here is a threshold.

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
from time_filter import stats, timed  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000, help="pairs the table is counted from (bench.py: 10 M)")
    ap.add_argument("--fastq-pairs", type=int, default=1_000_000, help="pairs written as FASTQ and corrected (692 bytes each)")
    ap.add_argument("--load", type=float, default=0.6)
    ap.add_argument("--lower", type=int, default=2, help="the count window is [lower, none]")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "time_correct.json"))
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
           "log2_bucket": table.log2_bucket, "table_bytes": table.nbytes, "lower": a.lower, "warmup": a.warmup, "reps": a.reps,
           "piece_bytes": fastqtext.piece_bytes()}
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        fq, out = os.path.join(tmp, "reads.fq"), os.path.join(tmp, "corrected.fq")
        synth.write_fastq_fast(s, cfg, fq, n_fq)
        del s
        data = np.fromfile(fq, dtype=np.uint8)
        n = int(data.size)
        text = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        text[:n] = torch.from_numpy(data).to(dev)
        del data
        res["text_bytes"] = n
        sp = _stream_ptr(dev)
        idx, n_lines = fastqtext.line_index(text, n)
        n_rec = n_lines // 4
        assert n_lines == 8 * n_fq
        status = torch.zeros(2, dtype=torch.int64, device=dev)
        # the yardstick: the spans kernel on the same text and window, and a copy of the same bytes
        spans = torch.empty((n_rec, 4), dtype=torch.int32, device=dev)
        sizes = torch.empty(n_rec, dtype=torch.int64, device=dev)
        spans_ms = timed(lambda: _lib.check(L.pg_table_read_spans(table.desc(), k, text.data_ptr(), n, idx.data_ptr(), n_rec, 0, a.lower, -1, 1, 0,
                                                                  _lib.SPAN_LONGEST, spans.data_ptr(), sizes.data_ptr(), status.data_ptr(), sp)),
                         a.warmup, a.reps)
        assert status.tolist() == [0, -1]
        res["spans"] = stats(spans_ms)
        res["spans_spread"] = round((max(spans_ms) - min(spans_ms)) / med(spans_ms), 4)
        copy = torch.empty_like(text)
        res["copy"] = stats(timed(lambda: copy.copy_(text), a.warmup, a.reps))
        # the three forms of the entry
        rows = torch.empty((n_rec, 4), dtype=torch.int32, device=dev)

        def call(out_ptr):
            _lib.check(L.pg_table_correct_reads(table.desc(), k, text.data_ptr(), n, idx.data_ptr(), n_rec, 0, a.lower, -1, 1, 0, out_ptr,
                                                rows.data_ptr(), status.data_ptr(), sp))

        res["correct_over_spans"] = {}
        ms = timed(lambda: call(None), a.warmup, a.reps)
        assert status.tolist() == [0, -1] and torch.equal(rows[:, :2], spans[:, :2])
        first = rows.clone()
        res["correct_rows"] = stats(ms)
        res["correct_over_spans"]["rows"] = round(med(ms) / med(spans_ms), 4)
        ms = timed(lambda: call(copy.data_ptr()), a.warmup, a.reps)         # (copy holds the text: every call stores the same bytes again)
        assert torch.equal(rows, first)
        changed = int((copy[:n] != text[:n]).sum())
        res["correct_out"] = stats(ms)
        res["correct_over_spans"]["out"] = round(med(ms) / med(spans_ms), 4)
        fixed = copy.clone()
        ms = []
        for i in range(a.warmup + a.reps):
            copy.copy_(text)                                                # (the text as it came, in the buffer that is corrected in place)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(L.pg_table_correct_reads(table.desc(), k, copy.data_ptr(), n, idx.data_ptr(), n_rec, 0, a.lower, -1, 1, 0, copy.data_ptr(),
                                                rows.data_ptr(), status.data_ptr(), sp))
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        assert torch.equal(rows, first) and torch.equal(copy[:n], fixed[:n])
        res["correct_in_place"] = stats(ms)
        res["correct_over_spans"]["in_place"] = round(med(ms) / med(spans_ms), 4)
        wide = first.to(torch.int64) & 0xFFFFFFFF
        candidates, corrected = int(wide[:, 2].sum()), int(wide[:, 3].sum())
        assert changed == corrected
        res["kmers"], res["hits_total"] = int(wide[:, 0].sum()), int(wide[:, 1].sum())
        res["candidates"], res["corrected"], res["reads_corrected"] = candidates, corrected, int((wide[:, 3] > 0).sum())
        res["candidates_per_read"], res["corrected_per_read"] = round(candidates / n_rec, 4), round(corrected / n_rec, 4)
        del text, idx, copy, fixed, spans, sizes, rows, first, wide
        # the whole call, file to file (the page cache holds the file: it was written a moment ago)
        calls = []
        for _ in range(a.warmup + a.reps):
            calls.append(table.correct_fastq(fq, out, lower=a.lower))
        calls = calls[a.warmup:]
        res["whole_call"] = {"seconds": stats([1000 * c["seconds"] for c in calls]), "device_ms": stats([c["device_ms"] for c in calls]),
                             "totals": {n_: calls[-1][n_] for n_ in ("records", "bases", "kmers", "hits", "candidates", "corrected", "reads_corrected")},
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
