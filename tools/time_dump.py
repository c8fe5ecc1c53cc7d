#!/usr/bin/env python3
"""The dump kernels on the table of the bench workload (BASELINE config 2: 10 M pairs, k = 21, a mini table sized as bench.py
sizes it), timed after warm-up, several repeats, median / min / max:

  writer   pg_table_dump_sizes + pg_table_dump_text over the whole table (device events), beside a plain device copy that moves
           the same number of bytes (the table read + the text written; a copy of half that many bytes reads and writes them);
  parser   pg_dump_parse of that text (device events), beside a device copy of the text;
  files    wall time of KmerTable.write_dump / KmerTable.from_dump to and from --dir (default /dev/shm) for a table cut down to
           --lines entries, beside the host path they replace on the same entries: items() + a numpy / Python formatter for
           writing, cli.load_dump + from_items for reading.

Prints one JSON document and writes it to --out.  Not a test: nothing here is a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pangaea_amd import _lib, cli, kmer, synth  # noqa: E402
from tools.time_inspect import stats, timed  # noqa: E402


def wall(f, warmup: int, reps: int) -> list:
    """milliseconds of wall time of ``reps`` calls of f (each ends synchronised), after ``warmup`` calls"""
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def host_write(table, path: str) -> None:
    """what the parent had for writing a dump: items() (host copies, numpy inverse hash, argsort) and a formatter"""
    codes, counts = table.items()
    k = table.k
    shifts = (2 * np.arange(k - 1, -1, -1)).astype(np.uint64)
    chars = np.frombuffer(b"ACTG", dtype=np.uint8)[((codes[:, None] >> shifts) & np.uint64(3)).astype(np.intp)]
    kmers = np.ascontiguousarray(chars).view(f"S{k}").ravel()
    with open(path, "wb") as f:
        f.write(b"".join(b"%s\t%d\n" % (a, b) for a, b in zip(kmers.tolist(), counts.tolist())))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--load", type=float, default=0.6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "time_dump.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k = 21
    cfg = synth.SynthConfig(n_pairs=a.pairs, n_barcodes=max(1, a.pairs // 200), read_len=150, seed=2022)
    s = synth.generate(cfg, device=dev, chunk_pairs=1 << 17, with_names=False)
    hint = max(1 << 14, int(1.05 * kmer.estimate_distinct(s, k)))
    table = kmer.KmerTable.alloc(k, dev, "mini", distinct_hint=hint, load=a.load).count(s)
    del s
    table.release_workspaces()
    lib = _lib.load()
    stream = kmer._stream_ptr(dev)
    res = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "k": k, "kind": table.kind, "log2_slots": table.log2_slots,
           "log2_bucket": table.log2_bucket, "table_bytes": table.nbytes, "unit_slots": _lib.DUMP_UNIT_SLOTS}

    # ---- writer: both passes over the whole table
    n_units = lib.pg_table_dump_units(table.desc())
    sizes = torch.empty((2, n_units), dtype=torch.int64, device=dev)

    def pass1():
        _lib.check(lib.pg_table_dump_sizes(table.desc(), 1, sizes[0].data_ptr(), sizes[1].data_ptr(), stream))

    p1 = timed(pass1, a.warmup, a.reps)
    offsets = torch.cat([sizes.new_zeros(1), torch.cumsum(sizes[0], 0)])
    total, lines = int(offsets[-1]), int(sizes[1].sum())
    text = torch.empty(total, dtype=torch.uint8, device=dev)

    def pass2():
        _lib.check(lib.pg_table_dump_text(table.desc(), 1, 0, n_units, offsets.data_ptr(), 0, total, text.data_ptr(), total, stream))

    p2 = timed(pass2, a.warmup, a.reps)
    moved = table.nbytes + total
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    cp = timed(lambda: dst.copy_(src), a.warmup, a.reps)
    del src, dst
    med = lambda v: sorted(v)[len(v) // 2]
    res["writer"] = {"lines": lines, "text_bytes": total, "bytes_moved": moved, "sizes_pass": stats(p1), "text_pass": stats(p2),
                     "copy_of_bytes_moved": stats(cp), "both_passes_over_copy": round((med(p1) + med(p2)) / med(cp), 3),
                     "text_pass_GBps_of_text": round(total / (med(p2) * 1e-3) / 1e9, 1)}
    print(json.dumps(res["writer"]), flush=True)

    # ---- parser: the whole text in one call
    cap = total // (k + 2) + 1
    out = torch.empty((3, cap), dtype=torch.int64, device=dev)
    ws = torch.empty(_lib.check(lib.pg_dump_parse_workspace_bytes(total)), dtype=torch.uint8, device=dev)
    word = torch.empty(3, dtype=torch.int64, device=dev)

    def parse():
        _lib.check(lib.pg_dump_parse(text.data_ptr(), total, k, 0, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), cap,
                                     word.data_ptr(), word[2:].data_ptr(), ws.data_ptr(), ws.numel(), stream))

    pp = timed(parse, a.warmup, a.reps)
    kept, seen, status = (int(v) for v in word.cpu())
    assert (kept, seen, status) == (lines, lines, -1), (kept, seen, status, lines)
    dst = torch.empty_like(text)
    cp = timed(lambda: dst.copy_(text), a.warmup, a.reps)
    del dst
    res["parser"] = {"lines": lines, "text_bytes": total, "parse": stats(pp), "copy_of_text": stats(cp),
                     "parse_over_copy": round(med(pp) / med(cp), 3), "parse_GBps_of_text": round(total / (med(pp) * 1e-3) / 1e9, 1)}
    print(json.dumps(res["parser"]), flush=True)

    # ---- files: a table of --lines entries, this path and the host path it replaces
    n = min(a.lines, lines)
    small = kmer.KmerTable.from_items(k, out[0, :n].clone(), out[1, :n].clone(), dev)
    del out, text, ws, table
    torch.cuda.empty_cache()
    new_path, old_path = os.path.join(a.dir, f"time_dump.{os.getpid()}.new.dump"), os.path.join(a.dir, f"time_dump.{os.getpid()}.old.dump")
    try:
        w_new = wall(lambda: small.write_dump(new_path), 1, a.reps)
        r_new = wall(lambda: kmer.KmerTable.from_dump(new_path, k, dev), 1, a.reps)
        w_old = wall(lambda: host_write(small, old_path), 0, a.host_reps)
        r_old = wall(lambda: kmer.KmerTable.from_items(k, *cli.load_dump(new_path, k), dev), 0, a.host_reps)
        same = sorted(open(new_path, "rb").read().splitlines()) == sorted(open(old_path, "rb").read().splitlines())
        assert same, "the two writers disagree"
        back = kmer.KmerTable.from_dump(new_path, k, dev).items()
        assert all(np.array_equal(x, y) for x, y in zip(back, small.items())), "the file does not give the table back"
        res["files"] = {"lines": n, "file_bytes": os.path.getsize(new_path), "dir": a.dir, "kind": small.kind, "log2_slots": small.log2_slots,
                        "write_dump_wall": stats(w_new), "from_dump_wall": stats(r_new),
                        "host_items_and_formatter_wall": stats(w_old), "host_load_dump_and_from_items_wall": stats(r_old),
                        "write_speedup_over_host": round(med(w_old) / med(w_new), 2), "read_speedup_over_host": round(med(r_old) / med(r_new), 2)}
    finally:
        for p in (new_path, old_path):
            if os.path.exists(p):
                os.remove(p)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
