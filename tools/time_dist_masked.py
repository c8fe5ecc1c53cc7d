#!/usr/bin/env python3
"""One rank's share of the N-rank job on MASKED input, on ONE GPU in a one-rank RCCL group, at the geometry the N-rank job would use
(the union's sketch from all N shards): the masked super-k-mer form (dist.MiniSharded: count half, exchange, lookup half, rows) against
the key-partitioned form it replaces (deferred count of the union-sized hash table, exchange, rows by table lookups), as bench.py
--rehearse-dist rehearses them.  Masks:
  qual  bases below the quality threshold (the table leaves them out, the rows do not): about 11 % of the bases, most of them near
        the ends of the 150-character reads (6 % everywhere + a bump that decays over 8 characters from either end)
  soft  soft-masked bases counted with lowercase_is_base: --lower of the 32-character words lower case (runs, as repeat masking leaves)
Prints one JSON line per form: HIP-event times per step (best and median of --steps), and whether both forms gave the same rows
(--verify: rows that differ from the one-GPU pipeline's, per form).
The collectives' own time is not measured: a one-rank group moves nothing between GPUs."""
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
ap.add_argument("--world", type=int, default=8, help="ranks of the job whose share this is (sketches of the other shards)")
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--mask", choices=("qual", "soft", "none"), default="qual", help="none: plain input (the plain N-rank form), for comparison")
ap.add_argument("--lower", type=float, default=0.10, help="soft: fraction of words lower case")
ap.add_argument("--verify", action="store_true", help="compare both forms' rows with the one-GPU pipeline's (count_kmers + features)")
ap.add_argument("--a2a-chunk-bytes", type=int, default=0, help="bytes per RCCL all-to-all call (dist.A2A_CHUNK_BYTES; 1099511627776: one call)")
args = ap.parse_args()
if args.a2a_chunk_bytes:
    pdist.A2A_CHUNK_BYTES = args.a2a_chunk_bytes
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29613")
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
pdist.OWNER_MIN_WORLD = 1                 # the owner-partitioned exchange of 4+ ranks, as bench.py --rehearse-dist 8 runs it
K, WINDOW, VSIZE, MIN_LEN, READ_LEN = 21, 10, 400, 2000, 150
n_bc = args.barcodes or max(1, args.pairs // 200)
LC = args.mask == "soft"


def pack(mask: torch.Tensor) -> torch.Tensor:
    """[words, 32] bool -> int32 validity plane"""
    bits = (mask.to(torch.int64) << torch.arange(32, device=mask.device)).sum(dim=1)
    return torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32)


def masked(s, r: int):
    g = torch.Generator(device=dev)
    g.manual_seed(1000 + r)
    step = 1 << 22
    if args.mask == "none":
        return s
    if args.mask == "qual":
        lowq = torch.empty_like(s.valid)
        for w0 in range(0, s.n_words, step):
            w1 = min(s.n_words, w0 + step)
            pos = torch.arange(32 * w0, 32 * w1, device=dev) % (READ_LEN + 1)            # (a read and its separator)
            d = torch.minimum(pos, READ_LEN - 1 - pos).clamp(min=0).to(torch.float32)
            p = 0.06 + 0.45 * torch.exp(-d / 8.0)
            lowq[w0:w1] = pack((torch.rand(p.shape, device=dev, generator=g) < p).view(-1, 32)) & s.valid[w0:w1]
        s.valid_lowq = lowq
    else:
        words = torch.rand(s.n_words, device=dev, generator=g) < args.lower
        lower = torch.where(words, s.valid, torch.zeros_like(s.valid))
        s.valid, s.valid_lower = s.valid & ~lower, lower
    return s


def shard(r):
    cfg = synth.SynthConfig(n_pairs=args.pairs, n_barcodes=n_bc, read_len=READ_LEN, seed=2022, first_pair=r * args.pairs)
    return masked(synth.generate(cfg, device=dev, chunk_pairs=1 << 17, with_names=False), r)


def timed(step):
    times = []
    for i in range(args.steps + 1):                                # (the first step: workspaces and code objects)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        if i:
            times.append(e0.elapsed_time(e1))
    return {"best": round(min(times), 2), "median": round(sorted(times)[len(times) // 2], 2), "all": [round(t, 2) for t in times]}


try:
    t0 = time.perf_counter()
    stream = shard(0)
    rows = stream.rows(MIN_LEN)
    plan = kmer.Plan(rows, dev)
    regs = kmer.distinct_sketch(stream, K, lowercase_is_base=LC)          # the table plane
    local_t = kmer.sketch_estimate(regs)
    local_u = kmer.sketch_estimate(kmer.distinct_sketch(stream, K, plane=stream.union_valid(LC)))
    for r in range(1, args.world):
        other = shard(r)
        regs = torch.maximum(regs, kmer.distinct_sketch(other, K, lowercase_is_base=LC))
        del other
    torch.cuda.empty_cache()
    total = max(1 << 14, int(1.05 * kmer.sketch_estimate(regs)))
    setup_s = time.perf_counter() - t0
    base = {"pairs": args.pairs, "barcodes": n_bc, "rows": int(plan.n_rows), "world": args.world, "words": int(stream.n_words), "mask": args.mask}
    if args.mask == "qual":
        ones = lambda p: sum(int(((p.to(torch.int64) >> i) & 1).sum()) for i in range(32))
        base["lowq_of_bases"] = round(ones(stream.valid_lowq) / ones(stream.valid), 4)
    elif args.mask == "soft":
        base["lower_of_bases"] = round(args.lower, 4)

    # ---- the masked super-k-mer form
    log2_u, lb_u, lb_l = pdist.MiniSharded.geometry(total, int(1.1 * local_u), n_rows=plan.n_rows)
    assert log2_u - lb_u <= 16, "the union does not fit the super-k-mer geometry"
    ms = pdist.MiniSharded(K, dev, log2_u, lb_l, WINDOW, VSIZE, union_log2_bucket=lb_u, lowercase_is_base=LC,
                           masked=args.mask != "none")
    abd_m = torch.zeros((len(rows), VSIZE), dtype=torch.int32, device=dev)

    def step_mini():
        ms.local._mini_plan = None                         # (every step plans its batch, as bench.py --plan in-step)
        ms.count(stream, plan, check=False)
        kmer.features(stream, plan, k_tnf=None, table=ms.local, window=WINDOW, vsize=VSIZE, out_abd=abd_m)

    t_mini = timed(step_mini)
    ms.check_status()
    print(json.dumps(dict(base, what="masked super-k-mer form (count half, exchange in a one-rank RCCL group, lookup half, rows)",
                          geometry={"union_log2_slots": log2_u, "union_log2_bucket": lb_u, "local_log2_bucket": lb_l},
                          pieces=ms.pieces, step_ms=t_mini, setup_s=round(setup_s, 1))), flush=True)
    del ms
    torch.cuda.empty_cache()

    # ---- the key-partitioned form it replaces
    table = kmer.KmerTable.alloc(K, dev, "hash", distinct_hint=total, load=0.6)
    defer = pdist.deferred_group_for(table, int(1.1 * local_t))
    abd_k = torch.zeros((len(rows), VSIZE), dtype=torch.int32, device=dev)

    def step_keyed():
        table.reset()
        table.count(stream, check=False, rows=plan, deferred_group=defer if defer is not None and table.can_defer(stream.n_words) else None,
                    lowercase_is_base=LC)
        pdist._exchange_bucketed(table)                    # (the same launches and collectives in a one-rank group)
        kmer.features(stream, plan, k_tnf=None, table=table, window=WINDOW, vsize=VSIZE, out_abd=abd_k)

    t_keyed = timed(step_keyed)
    table.check_status()
    print(json.dumps(dict(base, what="key-partitioned form (deferred count, exchange in a one-rank RCCL group, rows)",
                          table_log2_slots=table.log2_slots, deferred_group=defer, step_ms=t_keyed,
                          same_rows=bool(torch.equal(abd_m, abd_k)))), flush=True)
    if args.verify:
        del table
        torch.cuda.empty_cache()
        one = kmer.count_kmers(stream, K, rows=plan, emit=(WINDOW, VSIZE), lowercase_is_base=LC)
        _, abd_1 = kmer.features(stream, plan, k_tnf=None, table=one, window=WINDOW, vsize=VSIZE)
        diff = lambda a: int((a != abd_1).any(dim=1).sum())
        print(json.dumps({"verify": "rows that differ from the one-GPU pipeline's", "mask": args.mask, "super_kmer_form": diff(abd_m),
                          "key_partitioned_form": diff(abd_k), "rows": int(plan.n_rows)}), flush=True)
finally:
    dist.destroy_process_group()
