#!/usr/bin/env python3
"""KmerTable.trim_fastq on the bench table: tools/time_filter.py's table and text -- a synth stream of --pairs read pairs (bench.py's
configuration: k = 21, mini table, load 0.6) is counted, its first --fastq-pairs pairs are written as interleaved FASTQ
(synth.write_fastq_fast) -- and on that text, under the count window [--lower, none] (2: k-mers seen once are the errors'),

  spans_first    pg_table_read_spans, PG_SPAN_FIRST    (one wavefront per record: n, h and the run that begins at position 0)
  spans_longest  pg_table_read_spans, PG_SPAN_LONGEST  (... and the longest run)
  gather         pg_fastq_gather_trimmed               (the records whose longest span has k bases and more, cut to it)

are timed with device events after --warmup calls, --reps repeats, median [min - max]; then the whole call, file to file (wall
seconds and the device_ms it reports).  Two reference times from the same run stand beside them:

  hits           pg_table_read_hits on the same text and window: the kernel that already does the same staging and lookups
  gather_whole   pg_fastq_gather of the same kept records, untrimmed; both gathers also as nanoseconds per byte written

``spans_over_hits`` are the ratios of the medians, ``hits_spread`` the hits kernel's own (max - min) / median over its repeats: the
spans kernel adds a handful of wave-uniform steps per ballot word and 16 bytes out per record, so the expectation is a ratio
within 1 + spread.  Nothing here is a threshold.

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
    ap.add_argument("--fastq-pairs", type=int, default=1_000_000, help="pairs written as FASTQ and trimmed (692 bytes each)")
    ap.add_argument("--load", type=float, default=0.6)
    ap.add_argument("--lower", type=int, default=2, help="the count window is [lower, none]")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "time_trim.json"))
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
        fq, out = os.path.join(tmp, "reads.fq"), os.path.join(tmp, "trimmed.fq")
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
        # the parent's kernel on the same text and window
        hits = torch.empty((n_rec, 2), dtype=torch.int32, device=dev)
        hits_ms = timed(lambda: _lib.check(L.pg_table_read_hits(table.desc(), k, text.data_ptr(), n, idx.data_ptr(), n_rec, 0, a.lower, -1, 1, 0,
                                                                hits.data_ptr(), status.data_ptr(), sp)), a.warmup, a.reps)
        res["hits"] = stats(hits_ms)
        assert status.tolist() == [0, -1]
        res["hits_spread"] = round((max(hits_ms) - min(hits_ms)) / med(hits_ms), 4)
        # the spans, both modes (the longest last: its rows are the ones the gather takes)
        spans = torch.empty((n_rec, 4), dtype=torch.int32, device=dev)
        sizes = torch.empty(n_rec, dtype=torch.int64, device=dev)
        res["spans_over_hits"] = {}
        for name, mode in (("first", _lib.SPAN_FIRST), ("longest", _lib.SPAN_LONGEST)):
            ms = timed(lambda: _lib.check(L.pg_table_read_spans(table.desc(), k, text.data_ptr(), n, idx.data_ptr(), n_rec, 0, a.lower, -1, 1, 0, mode,
                                                                spans.data_ptr(), sizes.data_ptr(), status.data_ptr(), sp)), a.warmup, a.reps)
            assert status.tolist() == [0, -1] and torch.equal(spans[:, :2], hits)
            length = spans[:, 3].to(torch.int64)
            res["spans_" + name] = dict(stats(ms), with_span=int((length > 0).sum()), span_bases=int(length.sum()))
            res["spans_over_hits"][name] = round(med(ms) / med(hits_ms), 4)
        res["kmers"], res["hits_total"] = int(hits[:, 0].sum()), int(hits[:, 1].sum())
        # the two gathers of the same kept records
        kept = (spans[:, 3] >= k).nonzero().flatten()
        n_kept = int(kept.numel())
        whole = idx[4 * kept + 4] - idx[4 * kept]
        cut = sizes[kept]
        outbuf = torch.empty(max(int(whole.sum()), 16), dtype=torch.uint8, device=dev)
        for name, lens in (("gather", cut), ("gather_whole", whole)):
            dst = torch.cumsum(lens, 0) - lens
            total = int(lens.sum())
            if name == "gather":
                f = lambda: _lib.check(L.pg_fastq_gather_trimmed(text.data_ptr(), n, idx.data_ptr(), n_rec, kept.data_ptr(), spans.data_ptr(),   # noqa: E731
                                                                 dst.data_ptr(), n_kept, outbuf.data_ptr(), outbuf.numel(), sp))
            else:
                f = lambda: _lib.check(L.pg_fastq_gather(text.data_ptr(), n, idx.data_ptr(), n_rec, kept.data_ptr(), dst.data_ptr(), n_kept,     # noqa: E731
                                                         outbuf.data_ptr(), outbuf.numel(), sp))
            ms = timed(f, a.warmup, a.reps)
            res[name] = dict(stats(ms), kept_records=n_kept, bytes_written=total, ns_per_byte=round(1e6 * med(ms) / max(1, total), 6))
        res["gather"]["shortened_records"] = int((cut < whole).sum())
        res["gather_ns_per_byte_over_whole"] = round(res["gather"]["ns_per_byte"] / res["gather_whole"]["ns_per_byte"], 3)
        del text, idx, outbuf, spans, sizes, hits
        # the whole call, file to file (the page cache holds the file: it was written a moment ago)
        calls = []
        for _ in range(a.warmup + a.reps):
            calls.append(table.trim_fastq(fq, out, lower=a.lower, mode="longest", pair="both"))
        calls = calls[a.warmup:]
        res["whole_call"] = {"seconds": stats([1000 * c["seconds"] for c in calls]), "device_ms": stats([c["device_ms"] for c in calls]),
                             "totals": {n_: calls[-1][n_] for n_ in ("records", "kept", "passed", "trimmed", "bases", "bases_out", "kmers", "hits")},
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
