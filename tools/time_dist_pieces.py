#!/usr/bin/env python3
"""One rank's share of the N-rank super-k-mer form (dist.MiniSharded) on ONE GPU, in a one-rank RCCL group: the geometry the
N-rank job would use (the union's sketch from all N shards), then count half -> exchange -> lookup half -> rows per step.  Prints
one JSON line: the piece count the budget chose (or PANGAEA_MINI_PIECE_WORDS forced), the time per step (HIP events, best and
median of --steps), and the peak of device memory the steps allocated (torch's allocator: the stream and tables included)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from pangaea_amd import dist as pdist  # noqa: E402
from pangaea_amd import kmer, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=10_000_000, help="read pairs of this rank's share")
ap.add_argument("--barcodes", type=int, default=0, help="barcodes of the share (default: pairs / 200)")
ap.add_argument("--world", type=int, default=2, help="ranks of the job whose share this is (sketches of the other shards)")
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--piece-words", type=int, default=0, help="force words per piece (PANGAEA_MINI_PIECE_WORDS)")
args = ap.parse_args()
if args.piece_words:
    os.environ["PANGAEA_MINI_PIECE_WORDS"] = str(args.piece_words)
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29611")
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
K, WINDOW, VSIZE, MIN_LEN = 21, 10, 400, 2000
n_bc = args.barcodes or max(1, args.pairs // 200)


def shard(r):
    cfg = synth.SynthConfig(n_pairs=args.pairs, n_barcodes=n_bc, seed=2022, first_pair=r * args.pairs)
    return synth.generate(cfg, device=dev, chunk_pairs=1 << 17, with_names=False)


try:
    t0 = time.perf_counter()
    stream = shard(0)
    rows = stream.rows(MIN_LEN)
    plan = kmer.Plan(rows, dev)
    regs = kmer.distinct_sketch(stream, K)
    local = kmer.sketch_estimate(regs)
    for r in range(1, args.world):
        other = shard(r)
        regs = torch.maximum(regs, kmer.distinct_sketch(other, K))
        del other
    torch.cuda.empty_cache()
    total = max(1 << 14, int(1.05 * kmer.sketch_estimate(regs)))
    log2_u, lb_u, lb_l = pdist.MiniSharded.geometry(total, int(1.1 * local), n_rows=plan.n_rows)
    ms = pdist.MiniSharded(K, dev, log2_u, lb_l, WINDOW, VSIZE, union_log2_bucket=lb_u)
    abd = torch.zeros((len(rows), VSIZE), dtype=torch.int32, device=dev)
    setup_s = time.perf_counter() - t0
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    times = []
    for i in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms.local._mini_plan = None                         # (every step plans its batch, as bench.py --plan in-step)
        e0.record()
        ms.count(stream, plan, check=False)
        kmer.features(stream, plan, k_tnf=None, table=ms.local, window=WINDOW, vsize=VSIZE, out_abd=abd)
        e1.record()
        torch.cuda.synchronize()
        ms.check_status()
        times.append(e0.elapsed_time(e1))
    peak = torch.cuda.max_memory_allocated(dev)
    _, total_mem = torch.cuda.mem_get_info(dev)
    print(json.dumps({"what": "one rank's share of the N-rank super-k-mer form (count half, exchange in a one-rank RCCL group, lookup half, rows)",
                      "pairs": args.pairs, "barcodes": n_bc, "rows": int(plan.n_rows), "world": args.world, "words": int(stream.n_words),
                      "geometry": {"union_log2_slots": log2_u, "union_log2_bucket": lb_u, "local_log2_bucket": lb_l},
                      "pieces": ms.pieces, "forced_piece_words": args.piece_words or None,
                      "step_ms": {"best": round(min(times), 2), "median": round(sorted(times)[len(times) // 2], 2), "all": [round(t, 2) for t in times]},
                      "peak_alloc_gb": round(peak / 1e9, 2), "before_steps_gb": round(base / 1e9, 2), "device_gb": round(total_mem / 1e9, 1),
                      "setup_s": round(setup_s, 1)}), flush=True)
finally:
    dist.destroy_process_group()
