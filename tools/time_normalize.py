#!/usr/bin/env python3
"""KmerTable.normalize_fastq on the bench table: tools/time_filter.py's table and text -- a synth stream of --pairs read pairs
(bench.py's configuration: k = 21, mini table, load 0.6) is counted, its first --fastq-pairs pairs are written as interleaved
FASTQ (synth.write_fastq_fast) -- and on that text

  depths   pg_table_read_depths  (one wavefront per record: n, present, the lower median of its k-mers' counts, the pair's draw;
                                  every record of this text has at most 512 positions: the register form)
  hits     pg_table_read_hits    (window [1, none]) on the same text: the kernel of the same staging and lookups that this tool's
                                  subject does not touch

are timed with device events after --warmup calls, --reps repeats, median [min - max].  ``depths_over_hits`` is the ratio of the
medians, ``hits_spread`` the hits kernel's own (max - min) / median over its repeats.  The bench reads have no record over 512
positions, so a second text stands beside the first: --long-records records of --long-bases bases, each the sequence lines of
consecutive reads of the first text joined (what the table holds, with absent k-mers at the joints), on which the same two
entries are timed (``long``): there every record takes the radix-select form, one sweep for n, present and the maximum and one
per 8-bit digit of the answer.  Then the whole call, file to file (wall seconds and the device_ms it reports), with ``target`` =
half the median record depth of the first text, so that about half of it is kept.  Nothing here is a threshold.

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


def med(v):
    return sorted(v)[len(v) // 2]


def both_entries(table, text, n, a, L, sp) -> dict:
    """pg_table_read_hits and pg_table_read_depths on text[:n]: their times, the ratio, and what the rows say"""
    dev, k = text.device, table.k
    idx, n_lines = fastqtext.line_index(text, n)
    n_rec = n_lines // 4
    status = torch.zeros(2, dtype=torch.int64, device=dev)
    hits = torch.empty((n_rec, 2), dtype=torch.int32, device=dev)
    hits_ms = timed(lambda: _lib.check(L.pg_table_read_hits(table.desc(), k, text.data_ptr(), n, idx.data_ptr(), n_rec, 0, 1, -1, 1, 0, hits.data_ptr(),
                                                            status.data_ptr(), sp)), a.warmup, a.reps)
    assert status.tolist() == [0, -1]
    rows = torch.empty((n_rec, 4), dtype=torch.int32, device=dev)
    depths_ms = timed(lambda: _lib.check(L.pg_table_read_depths(table.desc(), k, text.data_ptr(), n, idx.data_ptr(), n_rec, 0, 1, 50, 1, 0, a.seed, 1,
                                                                rows.data_ptr(), status.data_ptr(), sp)), a.warmup, a.reps)
    assert status.tolist() == [0, -1]
    wide = rows.to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(wide[:, :2], hits.to(torch.int64) & 0xFFFFFFFF)           # (lower = 1: present is the hits of [1, none])
    d = wide[:, 2]
    return {"records": n_rec, "text_bytes": n, "hits": stats(hits_ms), "depths": stats(depths_ms),
            "depths_over_hits": round(med(depths_ms) / med(hits_ms), 4), "hits_spread": round((max(hits_ms) - min(hits_ms)) / med(hits_ms), 4),
            "kmers": int(wide[:, 0].sum()), "present": int(wide[:, 1].sum()), "max_positions": int(wide[:, 0].max()),
            "depth": {"median": int(d.median()), "max": int(d.max()), "mean": round(float(d.double().mean()), 3),
                      "digits": int(max(1, (int(d.max()).bit_length() + 7) // 8))}}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000, help="pairs the table is counted from (bench.py: 10 M)")
    ap.add_argument("--fastq-pairs", type=int, default=1_000_000, help="pairs written as FASTQ and normalised (692 bytes each)")
    ap.add_argument("--long-records", type=int, default=20_000, help="records of the second text")
    ap.add_argument("--long-bases", type=int, default=5000, help="bases of each of them")
    ap.add_argument("--load", type=float, default=0.6)
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "time_normalize.json"))
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
           "log2_bucket": table.log2_bucket, "table_bytes": table.nbytes, "seed": a.seed, "warmup": a.warmup, "reps": a.reps,
           "piece_bytes": fastqtext.piece_bytes()}
    with tempfile.TemporaryDirectory() as tmp:
        fq, out = os.path.join(tmp, "reads.fq"), os.path.join(tmp, "normalized.fq")
        synth.write_fastq_fast(s, cfg, fq, n_fq)
        del s
        data = np.fromfile(fq, dtype=np.uint8)
        n = int(data.size)
        text = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        text[:n] = torch.from_numpy(data).to(dev)
        sp = _stream_ptr(dev)
        res["short"] = both_entries(table, text, n, a, L, sp)
        assert res["short"]["records"] == 2 * n_fq and res["short"]["max_positions"] <= 512
        del text
        # the second text: sequence lines of consecutive reads joined into records of --long-bases bases
        per = -(-a.long_bases // 150)
        n_long = min(a.long_records, 2 * n_fq // per)
        head = bytes(data[:692 * ((n_long * per + 1) // 2)])
        del data
        seqs = head.split(b"\n")[1::4]
        assert len(seqs) >= n_long * per and all(len(x) == 150 for x in seqs[:per])
        quality = b"I" * a.long_bases
        long_text = b"".join(b"@long%d\n" % i + b"".join(seqs[per * i:per * i + per])[:a.long_bases] + b"\n+\n" + quality + b"\n" for i in range(n_long))
        n2 = len(long_text)
        text = torch.empty(n2 + 16, dtype=torch.uint8, device=dev)
        text[:n2] = torch.frombuffer(bytearray(long_text), dtype=torch.uint8).to(dev)
        del long_text, seqs, head
        res["long"] = dict(both_entries(table, text, n2, a, L, sp), bases_per_record=a.long_bases)
        assert res["long"]["max_positions"] > 512
        del text
        # the whole call, file to file (the page cache holds the file: it was written a moment ago)
        target = max(1, res["short"]["depth"]["median"] // 2)
        calls = []
        for _ in range(a.warmup + a.reps):
            calls.append(table.normalize_fastq(fq, out, target=target, seed=a.seed))
        calls = calls[a.warmup:]
        res["whole_call"] = {"target": target, "seconds": stats([1000 * c["seconds"] for c in calls]), "device_ms": stats([c["device_ms"] for c in calls]),
                             "totals": {n_: calls[-1][n_] for n_ in ("records", "kept", "passed", "low", "bases", "kmers", "hits", "depth_in", "depth_out")},
                             "kept_share": round(calls[-1]["kept"] / calls[-1]["records"], 4), "out_bytes": os.path.getsize(out)}
        res["whole_call"]["seconds"] = {n_.replace("_ms", "_s"): round(v / 1000, 4) if n_ != "reps" else v for n_, v in res["whole_call"]["seconds"].items()}
    text_out = json.dumps(res, indent=1)
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text_out + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
