#!/usr/bin/env python3
"""The table merge on two tables of the bench workload (BASELINE config 2: k = 21, mini tables of 2^16 buckets x 2^13 slots), each
counted from its own batch of 10 M synthetic pairs (two lanes of one sample: the same community, other pairs), timed after
warm-up, several repeats, median / min / max, beside a plain device copy that moves the same number of bytes (two tables read,
one written; a copy of half that many bytes reads and writes them):

  aligned   pg_table_merge_aligned of the two into a third table of their geometry (one workgroup per bucket, inside LDS);
  general   pg_table_merge of each into a cleared table of the same size (global compare-and-swap per entry; the clear is timed);
  today     what the parent had: dst.merge(src.compact()) into a copy of the first table (the copy is not timed).

Prints one JSON document and writes it to --out.  Not a test: nothing here is a threshold."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pangaea_amd import _lib, kmer, synth  # noqa: E402
from tools.time_inspect import stats, timed  # noqa: E402


def timed_after(setup, f, warmup: int, reps: int) -> list:
    """as ``timed``, with an untimed ``setup()`` in front of every call of f"""
    out = []
    for i in range(warmup + reps):
        setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--log2-slots", type=int, default=29)
    ap.add_argument("--log2-bucket", type=int, default=13)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "time_merge.json"))
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
           "log2_bucket": A.log2_bucket, "table_bytes": A.nbytes, "entries": [A._n_occupied(), B._n_occupied()]}
    med = lambda v: sorted(v)[len(v) // 2]

    # ---- the copy that moves the same bytes
    moved = 3 * A.nbytes
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    cp = timed(lambda: dst.copy_(src), a.warmup, a.reps)
    del src, dst
    res["bytes_moved"] = moved
    res["copy_of_bytes_moved"] = stats(cp)

    # ---- aligned
    out = kmer.KmerTable(k, "mini", torch.empty(1 << A.log2_slots, dtype=torch.int64, device=dev), A.log2_slots, A.log2_bucket)
    srcs = (C.POINTER(_lib.pg_table) * 2)(C.pointer(A._desc), C.pointer(B._desc))
    assert lib.pg_table_merge_aligned_applies(A.desc(), B.desc()) == 1

    def aligned():
        _lib.check(lib.pg_table_merge_aligned(out.desc(), srcs, 2, out.status.data_ptr(), stream))

    al = timed(aligned, a.warmup, a.reps)
    full = bool(int(out.status[0].item()) & _lib.STATUS_TABLE_FULL)
    out._empty = False
    res["aligned"] = {"merge": stats(al), "table_full": full, "entries": out._n_occupied(), "over_copy": round(med(al) / med(cp), 3),
                      "GBps_of_bytes_moved": round(moved / (med(al) * 1e-3) / 1e9, 1)}
    print(json.dumps(res["aligned"]), flush=True)
    spectrum = None if full else out.spectrum(1000)

    # ---- general, into a cleared table of the same size
    gen_t = kmer.KmerTable.mini_with_slots(k, dev, A.log2_slots, A.log2_bucket)

    def general():
        gen_t.data.zero_()
        _lib.check(lib.pg_table_merge(gen_t.desc(), A.desc(), gen_t.status.data_ptr(), stream))
        _lib.check(lib.pg_table_merge(gen_t.desc(), B.desc(), gen_t.status.data_ptr(), stream))

    ge = timed(general, a.warmup, a.reps)
    gen_t._empty = False
    gfull = bool(int(gen_t.status[0].item()) & _lib.STATUS_TABLE_FULL)
    res["general"] = {"clear_and_two_merges": stats(ge), "table_full": gfull, "entries": gen_t._n_occupied(), "over_copy": round(med(ge) / med(cp), 3),
                      "over_aligned": round(med(ge) / med(al), 3)}
    if spectrum is not None and not gfull:
        assert np.array_equal(gen_t.spectrum(1000), spectrum), "the two forms disagree"
        res["general"]["same_spectrum_as_aligned"] = True
    print(json.dumps(res["general"]), flush=True)
    del gen_t, out

    # ---- today's route: a copy of A, B's occupied slots compacted and added one compare-and-swap each
    today_t = kmer.KmerTable.mini_with_slots(k, dev, A.log2_slots, A.log2_bucket)
    today_t._empty = False

    def today():
        today_t.merge(B.compact(), check=False)

    to = timed_after(lambda: today_t.data.copy_(A.data), today, min(a.warmup, 1), a.reps)
    tfull = bool(int(today_t.status[0].item()) & _lib.STATUS_TABLE_FULL)
    res["today"] = {"compact_and_merge": stats(to), "table_full": tfull, "over_copy": round(med(to) / med(cp), 3), "over_aligned": round(med(to) / med(al), 3)}
    if spectrum is not None and not tfull:
        assert np.array_equal(today_t.spectrum(1000), spectrum), "today's route disagrees"
        res["today"]["same_spectrum_as_aligned"] = True
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
