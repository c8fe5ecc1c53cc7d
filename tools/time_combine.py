#!/usr/bin/env python3
"""The table combine (min, max, diff, left, only, keep) on two tables of the bench workload (BASELINE config 2: k = 21, mini tables
of 2^16 buckets x 2^13 slots), each counted from its own batch of 10 M synthetic pairs (two lanes of one sample: the same
community, other pairs), timed after warm-up, several repeats, median / min / max, beside a plain device copy that moves the bytes
of two tables read and one written (a copy of half that many bytes reads and writes them).  For every op:

  aligned   pg_table_combine_aligned of the two into a third table of their geometry (one workgroup per bucket, inside LDS);
  general   the general form of KmerTable.combined: the entries counted, pg_table_combine_items, a table from the items;
  today     what the parent offers through its public API: B.query(codes of A) on device tensors, torch arithmetic, from_items.

``keep`` is timed with lower = 2 (the solid k-mers), the others with the whole window.  Prints one JSON document and writes it to
--out (after every op, so that a run cut short leaves what it measured).  Not a test: nothing here is a threshold."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pangaea_amd import _lib, kmer, synth  # noqa: E402
from tools.time_inspect import stats, timed  # noqa: E402

OPS = ("min", "max", "diff", "left", "only", "keep")


def today(A, B, op: str, lower: int):
    """the op with what the parent has: the occupied slots of A to (code, count) tensors, B asked for A's codes, torch arithmetic,
    a table from the items that stay (max: B's own k-mers as well, by asking A for B's codes)"""
    cmask = (1 << _lib.HASH_COUNT_BITS) - 1
    kmask = (1 << (2 * A.k)) - 1

    def entries(t):
        s = t.compact()
        return (s >> _lib.HASH_COUNT_BITS) & kmask, s & cmask

    codes, ca = entries(A)
    cb = B.query(codes) if op != "keep" else None
    r = {"min": lambda: torch.minimum(ca, cb), "max": lambda: torch.maximum(ca, cb), "diff": lambda: torch.clamp(ca - cb, min=0),
         "left": lambda: torch.where(cb > 0, ca, 0), "only": lambda: torch.where(cb == 0, ca, 0), "keep": lambda: ca}[op]()
    if op == "max":
        codes_b, n_b = entries(B)
        own = A.query(codes_b) == 0
        codes, r = torch.cat([codes, codes_b[own]]), torch.cat([r, n_b[own]])
    keep = r >= lower
    return kmer.KmerTable.from_items(A.k, codes[keep], r[keep], A.device, kind="mini")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--log2-slots", type=int, default=29)
    ap.add_argument("--log2-bucket", type=int, default=13)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ops", default=",".join(OPS))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "time_combine.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k = 21
    lib = _lib.load()
    stream = kmer._stream_ptr(dev)
    tables = []
    for lane in range(2):
        cfg = synth.SynthConfig(n_pairs=a.pairs, n_barcodes=max(1, a.pairs // 200), read_len=150, seed=2022, first_pair=lane * a.pairs)
        s = synth.generate(cfg, device=dev, chunk_pairs=1 << 17, with_names=False)
        t = kmer.KmerTable.mini_with_slots(k, dev, a.log2_slots, a.log2_bucket).count(s)
        del s
        t.release_workspaces()
        tables.append(t)
    A, B = tables
    res = {"device": torch.cuda.get_device_name(0), "pairs_per_table": a.pairs, "k": k, "kind": A.kind, "log2_slots": A.log2_slots,
           "log2_bucket": A.log2_bucket, "table_bytes": A.nbytes, "entries": [A._n_occupied(), B._n_occupied()], "compare": A.compare(B)}
    med = lambda v: sorted(v)[len(v) // 2]

    def save():
        text = json.dumps(res, indent=1)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
        return text

    # ---- the copy that moves the same bytes
    moved = 3 * A.nbytes
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    cp = timed(lambda: dst.copy_(src), a.warmup, a.reps)
    del src, dst
    res["bytes_moved"] = moved
    res["copy_of_bytes_moved"] = stats(cp)
    cmp_ms = timed(lambda: A.compare(B), a.warmup, a.reps)
    res["compare_two_passes"] = stats(cmp_ms)
    print(json.dumps({"copy": res["copy_of_bytes_moved"], "compare": res["compare_two_passes"]}), flush=True)

    out = kmer.KmerTable(k, "mini", torch.empty(1 << A.log2_slots, dtype=torch.int64, device=dev), A.log2_slots, A.log2_bucket)
    assert lib.pg_table_merge_aligned_applies(A.desc(), B.desc()) == 1
    res["ops"] = {}
    for op in [o for o in a.ops.split(",") if o]:
        lower = 2 if op == "keep" else 1
        other = None if op == "keep" else B
        row = res["ops"][op] = {"lower": lower}

        def aligned():
            _lib.check(lib.pg_table_combine_aligned(out.desc(), A.desc(), None if other is None else other.desc(), _lib.COMBINE_OPS[op], lower, -1,
                                                    out.status.data_ptr(), stream))

        out.status.zero_()
        al = timed(aligned, a.warmup, a.reps)
        full = bool(int(out.status[0].item()) & _lib.STATUS_TABLE_FULL)
        out._empty = False
        spectrum = None if full else out.spectrum(1000)
        row["aligned"] = {"combine": stats(al), "table_full": full, "entries": out._n_occupied(), "over_copy": round(med(al) / med(cp), 3),
                          "GBps_of_bytes_moved": round((moved if other is not None else 2 * A.nbytes) / (med(al) * 1e-3) / 1e9, 1)}
        print(op, json.dumps(row["aligned"]), flush=True)

        held = []

        def general():
            held[:] = [kmer.KmerTable._combined_general(A, other, op, "mini", lower, -1)]

        ge = timed(general, a.warmup, a.reps)
        row["general"] = {"count_items_and_table": stats(ge), "log2_slots": held[0].log2_slots, "over_copy": round(med(ge) / med(cp), 3),
                          "over_aligned": round(med(ge) / med(al), 3)}
        if spectrum is not None:
            assert np.array_equal(held[0].spectrum(1000), spectrum), "the two forms disagree"
            row["general"]["same_spectrum_as_aligned"] = True
        print(op, json.dumps(row["general"]), flush=True)
        held.clear()

        def parent():
            held[:] = [today(A, B, op, lower)]

        try:
            to = timed(parent, min(a.warmup, 1), a.reps)
            row["today"] = {"query_torch_from_items": stats(to), "log2_slots": held[0].log2_slots, "over_copy": round(med(to) / med(cp), 3),
                            "over_aligned": round(med(to) / med(al), 3)}
            if spectrum is not None:
                assert np.array_equal(held[0].spectrum(1000), spectrum), "today's route disagrees"
                row["today"]["same_spectrum_as_aligned"] = True
        except _lib.PangaeaError as e:                 # (from_items sizes the table for the items and does not grow it)
            row["today"] = {"failed": str(e)}
        print(op, json.dumps(row["today"]), flush=True)
        held.clear()
        torch.cuda.empty_cache()
        save()
    print(save())
    return 0


if __name__ == "__main__":
    sys.exit(main())
