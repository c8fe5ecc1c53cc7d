#!/usr/bin/env python3
"""prepreads.preprocess_reads and the one-call prepared sort on synthetic raw reads: N_PAIRS read pairs (bench.py's data: 150-base
reads, 200 pairs per barcode, 2 % without a barcode; the pairs in a random order, a fixed seed) are written twice --

  stlfr    R1 / R2 with ``@r<8 digits>#<b1>_<b2>_<b3>/<mate>`` headers (four digits per field; ``#0_0_0`` without a barcode)
  tellseq  R1 / R2 with ``@r<8 digits> <mate>:N:0:ACGT`` headers and I1 with 18-base index reads (17 bases where the pair has no
           barcode: such a pair is dropped)

-- and on those texts, in one process, entry by entry with device events after --warmup calls, --reps repeats, median [min - max]:

  plan        pg_fastq_prep_plan   (one wavefront per unit: where the barcode lies, tagged / kept, the status rows)
  lengths     the new records' bytes and their scan (torch, element-wise on the line indices and the plan arrays)
  write       pg_fastq_prep_write  (both mates' new records to their places; two buffers, and one interleaved buffer)

beside the yardsticks, which are unchanged from the sort:

  tags        pg_fastq_barcode_tags on R1 (lines_per_unit 4): what the plan kernel is compared with
  gather      pg_fastq_gather of all records of R1 and R2 in input order into one buffer: what the write kernel is compared with
  copy        a device copy of as many bytes as the write kernel writes

then wall seconds of ``preprocess_reads`` (files to files), of the one-call prepared sort (``sort_fastq(short_type=...)``) and of the
two-step route (``preprocess_reads`` to files, then ``sort_fastq -1 -2`` on them), with the per-stage device_ms they report.
``plan_over_tags`` and ``write_over_gather_per_byte`` are ratios of medians.  Nothing here is a threshold.

Prints one JSON document and writes it to --out."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pangaea_amd import _lib, fastqtext, prepreads, sortreads, synth  # noqa: E402


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


def med(v: list) -> float:
    return sorted(v)[len(v) // 2]


def _digits(v: np.ndarray, width: int) -> np.ndarray:
    return np.stack([(v // 10 ** (width - 1 - i)) % 10 + 48 for i in range(width)], 1).astype(np.uint8)


def _const(text: bytes, rows: int) -> np.ndarray:
    return np.broadcast_to(np.frombuffer(text, dtype=np.uint8), (rows, len(text)))


def make_inputs(pairs: int, seed: int, tmp: str, device) -> dict:
    """the raw files of both libraries, from one synthetic data set: {"stlfr": [R1, R2], "tellseq": [R1, R2, I1]} (paths)"""
    cfg = synth.SynthConfig(n_pairs=pairs, n_barcodes=max(1, pairs // 200), read_len=150, seed=seed)
    L, P = cfg.read_len, cfg.pairs_per_barcode
    made = os.path.join(tmp, "made.fq")
    s = synth.generate(cfg, device=device, chunk_pairs=1 << 17, with_names=False)
    synth.write_fastq_fast(s, cfg, made)
    del s
    n_bc = min(pairs, P * cfg.n_barcodes)
    raw = np.fromfile(made, dtype=np.uint8)
    os.remove(made)
    w_bc, w_no = 42 + 2 * L + 4, 11 + 2 * L + 4               # a record with / without a tag (synth.write_fastq_fast)
    assert raw.size == 2 * (n_bc * w_bc + (pairs - n_bc) * w_no)
    rng = np.random.RandomState(seed)
    blocks = []                                               # (the pairs' rows, the header's width, the pairs' barcodes or None)
    tagged = raw[:2 * n_bc * w_bc].reshape(n_bc, 2 * w_bc)[rng.permutation(n_bc)]
    plain = raw[2 * n_bc * w_bc:].reshape(pairs - n_bc, 2 * w_no)
    # the pairs in a random order: the tagged rows permuted, the others dealt between them in up to 64 runs
    cuts_t, cuts_p = np.linspace(0, n_bc, 65).astype(int), np.linspace(0, pairs - n_bc, 65).astype(int)
    for k in range(64):
        blocks.append((tagged[cuts_t[k]:cuts_t[k + 1]], 42, True))
        blocks.append((plain[cuts_p[k]:cuts_p[k + 1]], 11, False))
    outs = {"stlfr": [[], []], "tellseq": [[], [], []]}
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for rows, w, has in blocks:
        m = rows.shape[0]
        if not m:
            continue
        name = rows[:, :10]                                   # "@r" and eight digits
        body = [rows[:, w:w + 2 * L + 4], rows[:, 2 * w + 2 * L + 4:]]       # sequence, "+", quality with their line ends, per mate
        if has:
            b = np.zeros(m, dtype=np.int64)                   # the barcode's number: the seven digits behind the 16 bases of its name
            for i in range(7):
                b = b * 10 + (rows[:, 32 + i].astype(np.int64) - 48)
            fields = [_digits(b % 1536 + 1, 4), _const(b"_", m), _digits((b // 1536) % 1536 + 1, 4), _const(b"_", m), _digits(b // (1536 * 1536) + 1, 4)]
            index = np.concatenate([rows[:, 16:32], acgt[(b & 3)][:, None], acgt[((b >> 2) & 3)][:, None]], 1)
        else:
            fields = [_const(b"0_0_0", m)]
            index = _const(b"N" * 17, m)
        for mate in (0, 1):
            outs["stlfr"][mate].append(np.concatenate([name, _const(b"#", m), *fields, _const(b"/%d\n" % (mate + 1), m), body[mate]], 1).reshape(-1))
            outs["tellseq"][mate].append(np.concatenate([name, _const(b" %d:N:0:ACGT\n" % (mate + 1), m), body[mate]], 1).reshape(-1))
        outs["tellseq"][2].append(np.concatenate([name, _const(b" 1:N:0\n", m), index, _const(b"\n+\n", m), _const(b"I" * index.shape[1], m),
                                                  _const(b"\n", m)], 1).reshape(-1))
    paths = {}
    for lib, files in outs.items():
        paths[lib] = []
        for name, parts in zip(("R1", "R2", "I1"), files):
            paths[lib].append(os.path.join(tmp, f"{lib}_{name}.fq"))
            with open(paths[lib][-1], "wb") as f:
                for part in parts:
                    part.tofile(f)
    return paths


def measure(lib: str, files: list, pairs: int, tmp: str, a) -> dict:
    dev = torch.device("cuda:0")
    mode = _lib.PREP_MODES[lib]
    res = {"files_bytes": [os.path.getsize(f) for f in files]}
    texts, sizes, idxs = [], [], []
    for f in files:
        text, n = sortreads._read_text(f, dev)
        idx, n_lines = sortreads.line_index(text, n)
        assert n_lines == 4 * pairs
        texts.append(text)
        sizes.append(n)
        idxs.append(idx)
    plan_ms = timed(lambda: prepreads.Plan(mode, texts, sizes, idxs, pairs), a.warmup, a.reps)
    plan = prepreads.Plan(mode, texts, sizes, idxs, pairs)
    assert prepreads.status_error(files, plan.status) is None
    flagged = int(plan.tagged.sum())
    header_bytes = int((idxs[0][1:4 * pairs:4] - idxs[0][0:4 * pairs:4]).sum())
    res["plan"] = dict(stats(plan_ms), units=pairs, flagged=flagged, header_bytes=header_bytes)
    tags_ms = timed(lambda: sortreads.barcode_tags(texts[0], idxs[0], pairs, 4, sizes[0]), a.warmup, a.reps)
    res["tags"] = stats(tags_ms)

    def lengths():
        kept = plan.kept()
        len1, len2 = plan.record_bytes(kept)
        return kept, len1, len2, torch.cumsum(len1, 0) - len1, torch.cumsum(len2, 0) - len2

    res["lengths"] = stats(timed(lengths, a.warmup, a.reps))
    kept, len1, len2, at1, at2 = lengths()
    n1, n2 = int(len1.sum()), int(len2.sum())
    n_kept = int(len1.numel())
    out = torch.empty(n1 + n2 + 64, dtype=torch.uint8, device=dev)
    wl = torch.empty(19 * n_kept, dtype=torch.uint8, device=dev) if mode == _lib.PREP_TELLSEQ else None
    two_ms = timed(lambda: plan.write(kept, at1, at2, out, n1, out[n1 + 32:], n2, wl), a.warmup, a.reps)
    both = len1 + len2
    at = torch.cumsum(both, 0) - both
    at_2 = at + len1
    one_ms = timed(lambda: plan.write(kept, at, at_2, out, n1 + n2, out, n1 + n2), a.warmup, a.reps)
    res["write_two_files"] = dict(stats(two_ms), units=n_kept, bytes=n1 + n2 + (19 * n_kept if wl is not None else 0))
    res["write_interleaved"] = dict(stats(one_ms), units=n_kept, bytes=n1 + n2)
    # the yardsticks: every record of R1 and R2 as it is, in input order, into one buffer; a copy of the bytes written
    raw = sizes[0] + sizes[1]
    big = torch.empty(max(raw, n1 + n2) + 64, dtype=torch.uint8, device=dev)
    gplan = sortreads._gather_plan(texts[:2], sizes[:2], idxs[:2], torch.arange(pairs, dtype=torch.int64, device=dev))
    gather_ms = timed(lambda: sortreads._gather_run(gplan, big, raw), a.warmup, a.reps)
    res["gather"] = dict(stats(gather_ms), records=2 * pairs, bytes=raw)
    copy_ms = timed(lambda: big[:n1 + n2].copy_(out[:n1 + n2]), a.warmup, a.reps)
    res["copy_written_bytes"] = dict(stats(copy_ms), bytes=n1 + n2)
    res["plan_over_tags"] = round(med(plan_ms) / med(tags_ms), 3)
    res["write_bytes_per_ms"] = round((n1 + n2) / med(one_ms))
    res["gather_bytes_per_ms"] = round(raw / med(gather_ms))
    res["write_over_gather_per_byte"] = round((med(one_ms) / (n1 + n2)) / (med(gather_ms) / raw), 3)
    res["write_over_copy"] = round(med(one_ms) / med(copy_ms), 3)
    del texts, idxs, plan, out, big, gplan, kept, len1, len2, at1, at2, at, at_2, both, wl
    torch.cuda.empty_cache()
    # whole calls, files to files (the page cache holds the files: they were written a moment ago)
    index = files[2] if len(files) == 3 else None
    pre, one, two = os.path.join(tmp, lib + ".pre"), os.path.join(tmp, lib + ".one.fq"), os.path.join(tmp, lib + ".two.fq")

    def seconds(calls: list, key: str = "seconds") -> dict:
        return {k.replace("_ms", "_s"): v for k, v in stats([c[key] for c in calls]).items()}

    def stages(calls: list) -> dict:
        return {stage: stats([c["device_ms"][stage] for c in calls]) for stage in calls[-1]["device_ms"]}

    calls = [prepreads.preprocess_reads(lib, files[0], files[1], pre, index=index) for _ in range(a.warmup + a.reps)][a.warmup:]
    res["preprocess_reads"] = {"seconds": seconds(calls), "device_ms": stages(calls),
                               "result": {k: v for k, v in calls[-1].items() if k not in ("seconds", "device_ms", "files")}}
    calls = [sortreads.sort_fastq(files[0], one, files[1], short_type=lib, index=index) for _ in range(a.warmup + a.reps)][a.warmup:]
    res["one_call_sort"] = {"seconds": seconds(calls), "device_ms": stages(calls),
                            "result": {k: v for k, v in calls[-1].items() if k not in ("seconds", "device_ms")}}
    steps = []
    for _ in range(a.warmup + a.reps):
        first = prepreads.preprocess_reads(lib, files[0], files[1], pre, index=index)
        second = sortreads.sort_fastq(pre + "_1.fq", two, pre + "_2.fq")
        steps.append({"seconds": first["seconds"] + second["seconds"], "preprocess_s": first["seconds"], "sort_s": second["seconds"]})
    steps = steps[a.warmup:]
    res["two_step_route"] = {"seconds": seconds(steps), "preprocess_seconds": seconds(steps, "preprocess_s"), "sort_seconds": seconds(steps, "sort_s")}
    with open(one, "rb") as f, open(two, "rb") as g:
        same = True
        while same:
            x, y = f.read(1 << 26), g.read(1 << 26)
            same = x == y
            if not x:
                break
    res["one_call_equals_two_step"] = bool(same)
    for f in (one, two, pre + "_1.fq", pre + "_2.fq", pre + ".wl"):
        if os.path.exists(f):
            os.remove(f)
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", nargs="?", type=int, default=1_000_000, help="read pairs (default 1 M)")
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "time_prep.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "seed": a.seed, "warmup": a.warmup, "reps": a.reps,
           "piece_bytes": fastqtext.piece_bytes()}
    with tempfile.TemporaryDirectory() as tmp:
        paths = make_inputs(a.pairs, a.seed, tmp, torch.device("cuda:0"))
        for lib in ("stlfr", "tellseq"):
            res[lib] = measure(lib, paths[lib], a.pairs, tmp, a)
    text_out = json.dumps(res, indent=1)
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text_out + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
