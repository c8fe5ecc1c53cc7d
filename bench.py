#!/usr/bin/env python3
"""bench.py -- read-pairs/s through the barcode feature path + VAE encode (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--pairs P] [--dump-outputs DIR] [--full [--no-cpu-baseline]]

One "step" = one pass of the hot path over one batch of synthetic barcoded read pairs that are already resident
in HBM in packed form: clear + build the global canonical 21-mer table (K2), exchange it between ranks (N > 1),
count TNF + abundance rows for every barcode (K1+K3), L1-normalise, VAE encode -> mu[N,32].
Workload at N=1 = BASELINE.json configs[1]: 10 M 150 bp pairs, 50 k barcodes, k=21, k_tnf=4, V=400, W=10.
For N > 1 every rank holds its own 10 M-pair shard of one N x 10 M-pair data set (weak scaling); launched as
``python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...``.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the steps and prints the line.  ``--full`` adds what takes runs of its own: the CPU
baseline (``cpu_baseline``) and the FASTQ file -> mu leg (``e2e``).  ``--dump-outputs DIR`` writes what the last timed
step computed (rank 0's) as DIR/<name>.npy, for an output-for-output comparison of two builds (``dump_outputs``).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

K_ABD, K_TNF, WINDOW, VSIZE, MIN_LEN, READ_LEN = 21, 4, 10, 400, 2000, 150
HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)

# Algorithmic bytes per read pair (restated in DESIGN.md), L=150, k=21, n_k = 2(L-k+1) = 260:
#   stream  : 302 characters x (2-bit code + 1-bit validity) = 113.25 B
#   K2 hash : stream + n_k x 16 B (8-B slot read + 8-B slot write-back)      = 4273.25 B
#   K3 hash : stream + n_k x 8 B (slot read) + (136+400) x 4 B / 200 pairs   = 2203.97 B
# One GPU runs K3's table lookups INSIDE the K2 kernel pass (a bucket's records are looked up while its counts are still in
# LDS): the n_k x 8 B of slot reads then belong to the stage that does them, "kmer_count+lookup"; what is left of K3 (row
# shuffle, row histograms, TNF) only owes the stream and the output rows.
STREAM_B = 302 * 3 / 8
ALG_BYTES = {"kmer_count": STREAM_B + 260 * 16, "features": STREAM_B + 260 * 8 + (136 + 400) * 4 / 200}
ALG_BYTES_FUSED = {"kmer_count+lookup": STREAM_B + 260 * 16 + 260 * 8, "features": STREAM_B + (136 + 400) * 4 / 200}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=10_000_000, help="read pairs per GPU (default: BASELINE config 2)")
    ap.add_argument("--barcodes", type=int, default=0, help="barcodes per GPU (default pairs/200)")
    ap.add_argument("--full", action="store_true", help="also the CPU baseline and the end-to-end leg (FASTQ file -> mu), reported beside the line's value")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32 / float64, at most 64 MB)")
    ap.add_argument("--cpu-sample", type=int, default=100_000, help="pairs in the CPU-baseline sample (--full)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--e2e-pairs", type=int, default=-1, help="pairs of the end-to-end leg (--full; FASTQ file -> mu); default: the whole workload; 0 = skip")
    ap.add_argument("--rehearse-dist", type=int, default=0, metavar="N",
                    help="one GPU: run the N-rank code path (deferred count, exchange over a one-rank RCCL group, table sized for N shards) -- not a result")
    ap.add_argument("--load", type=float, default=0.6, help="highest load of the hash table (its size is the next power of two)")
    ap.add_argument("--no-fuse", action="store_true", help="N = 1: separate count and lookup kernels (as N > 1 must run them)")
    ap.add_argument("--no-mini", action="store_true", help="N = 1: the key-partitioned pipeline (8-byte record per k-mer occurrence) instead of super-k-mers")
    ap.add_argument("--plan", choices=("ahead", "in-step", "once"), default="ahead",
                    help="super-k-mer pipeline, the partition plan of a batch (it depends on the reads, the rows and the table geometry): "
                         "'ahead' = computed in every step for the NEXT batch, on a side stream under the row histograms and the encode "
                         "of this one (default); 'in-step' = computed in front of the count of its own batch; 'once' = computed once, "
                         "before the timed steps (valid only because the bench repeats one batch: a comparison figure, never the default)")
    ap.add_argument("--no-defer", action="store_true", help="N > 1: write every rank's own table and compact it (instead of the deferred count)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (gloo lets several ranks rehearse on one GPU)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


# --dump-outputs: mu for at most 2^16 rows (8.4 MB), the TNF and abundance rows for at most 2^13 (35.1 MB) -- under 64 MB in all
DUMP_MU_ROWS, DUMP_FEATURE_ROWS, DUMP_SEED = 1 << 16, 1 << 13, 2022


def dump_rows(n: int, cap: int) -> np.ndarray:
    """the rows a dump keeps: all n when n <= cap, else a fixed seeded sample of cap rows (sorted; the same for the same n)"""
    if n <= cap:
        return np.arange(n)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n, cap, replace=False))


def dump_outputs(out_dir: str, mu, tnf, abd) -> None:
    """what the caller of one step receives: mu (float32, as computed) and the TNF / abundance rows it was encoded from (int32
    counts, written as float64: exact), each row-sampled by ``dump_rows`` when the batch is large"""
    os.makedirs(out_dir, exist_ok=True)
    n = mu.shape[0]
    for name, x, cap, dt in (("mu", mu, DUMP_MU_ROWS, torch.float32), ("tnf", tnf, DUMP_FEATURE_ROWS, torch.float64),
                             ("abd", abd, DUMP_FEATURE_ROWS, torch.float64)):
        assert x.shape[0] == n
        idx = torch.from_numpy(dump_rows(n, cap)).to(x.device)
        np.save(os.path.join(out_dir, f"{name}.npy"), x.index_select(0, idx).to(dt).cpu().numpy())


def cpu_baseline(stream, cfg, n_sample: int, state: dict) -> dict:
    """the reference's CPU path on the first n_sample pairs of the same workload, on this box's host cores:
    count_tnf + count_kmer are the REFERENCE binaries (oracle/_ref) when present, else the oracle port; the
    jellyfish stage (absent everywhere) is the oracle's exact counter; then data.py normalise + VAE encode."""
    from oracle import oracle
    from pangaea_amd import synth

    cores = min(len(os.sched_getaffinity(0)), 16)      # the one-GPU box's CPU share
    oracle.lib()
    tmp = tempfile.mkdtemp(prefix="pg_cpu_")
    fq = os.path.join(tmp, "sample.fq")
    n = synth.write_fastq(stream, cfg, fq, n_sample)
    ref_tnf, ref_kmer = oracle.ref_tool("count_tnf"), oracle.ref_tool("count_kmer")
    t = {}
    t0 = time.perf_counter()
    rd = oracle.Reads(fq)
    text = np.frombuffer(rd.all_seq(), dtype=np.uint8)
    t["parse(port)"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    table = oracle.Table(K_ABD, threads=cores).count(text)
    dump = os.path.join(tmp, "k.dump")
    table.dump(dump)
    t["jellyfish-standin(port)"] = time.perf_counter() - t0
    kind = "reference" if ref_tnf and ref_kmer else "port"
    if kind == "reference":
        t0 = time.perf_counter()
        subprocess.run([ref_tnf, "-i", fq, "-k", str(K_TNF), "-l", str(MIN_LEN), "-t", str(cores), "-o", os.path.join(tmp, "t.gz")],
                       check=True, stdout=subprocess.DEVNULL)
        t["count_tnf(reference)"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        subprocess.run([ref_kmer, "-i", fq, "-g", dump, "-k", str(K_ABD), "-l", str(MIN_LEN), "-w", str(WINDOW), "-v", str(VSIZE),
                        "-t", str(cores), "-o", os.path.join(tmp, "a.gz")], check=True, stdout=subprocess.DEVNULL)
        t["count_kmer(reference)"] = time.perf_counter() - t0
        names, tnf, abd = rd.features(MIN_LEN, k_tnf=K_TNF, k_abd=K_ABD, table=table, window=WINDOW, vsize=VSIZE, threads=cores)
    else:
        t0 = time.perf_counter()
        names, tnf, abd = rd.features(MIN_LEN, k_tnf=K_TNF, k_abd=K_ABD, table=table, window=WINDOW, vsize=VSIZE, threads=cores)
        t["count_tnf+count_kmer(port)"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    a, b, _ = oracle.data_normalize(abd, tnf)
    torch.set_num_threads(cores)
    oracle.vae_embedding(state, a, b)
    t["normalise+encode(torch cpu)"] = time.perf_counter() - t0
    counted = {k: v for k, v in t.items() if not k.startswith("parse")}
    total = sum(counted.values())
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
    return {"value": n / total, "unit": "pairs/s", "cores": cores, "kind": kind,
            "sample": f"first {n} pairs of the workload as FASTQ; seconds: " + ", ".join(f"{k} {v:.2f}" for k, v in counted.items())}


def e2e_leg(stream, cfg, n_pairs: int, vae, dev) -> dict:
    """the same path from a FASTQ FILE -- threaded ingest (parse, 2-bit pack, barcode runs), H2D copy, table
    sizing + partition plan + count with the lookups inside, TNF + abundance rows, L1-normalise, encode -> mu -- timed
    end to end on the first ``n_pairs`` pairs of the workload written as plain interleaved FASTQ (page cache: the file was
    just written).  Reported next to ``value``, never as it."""
    from pangaea_amd import kmer, synth
    from pangaea_amd.data import Data
    from pangaea_amd.reads import ReadStream

    tmp = tempfile.mkdtemp(prefix="pg_e2e_")
    fq, warm = os.path.join(tmp, "reads.fq"), os.path.join(tmp, "warm.fq")
    n = synth.write_fastq_fast(stream, cfg, fq, n_pairs)
    synth.write_fastq_fast(stream, cfg, warm, min(20_000, n_pairs))
    size = os.path.getsize(fq)
    os.sync()                                           # (the file has just been written: its write-back must not run under the timed passes)

    def run(path):
        lap = {}
        t0 = t = time.perf_counter()
        # (pg_ingest_fastq_device: the parser threads copy finished pieces to the GPU while the others parse on; the shift of the
        # pieces into place is a kernel.  PANGAEA_INGEST_ON_HOST=1: host ingest, then one copy)
        # (as feature.compute_features does: the pipeline's scratch is allocated by a helper thread while the host threads parse)
        warm = kmer.prewarm_workspaces(dev, int(os.path.getsize(path) / 690 * 1.03) + 1, K_ABD, VSIZE)
        s = ReadStream.from_fastq(path, device=dev)
        if warm is not None:
            warm.join()
        torch.cuda.synchronize()
        lap["ingest+h2d"] = time.perf_counter() - t; t = time.perf_counter()
        regs = kmer.distinct_sketch(s, K_ABD)                 # (the sizing pass runs on the GPU while the host builds the rows)
        rows = s.rows(MIN_LEN)
        plan = kmer.Plan(rows, dev)
        hint = max(1 << 13, int(1.1 * kmer.sketch_estimate(regs)))
        table = kmer.count_kmers(s, K_ABD, rows=plan, emit=(WINDOW, VSIZE), distinct_hint=hint, load=0.4)      # (allocation, partition plan, count + lookups)
        tnf, abd = kmer.features(s, plan, k_tnf=K_TNF, table=table, window=WINDOW, vsize=VSIZE)
        torch.cuda.synchronize()
        lap["table+rows"] = time.perf_counter() - t; t = time.perf_counter()
        mu = vae.encode(Data(np.array(rows.names, dtype=object), abd, tnf, device=dev))
        torch.cuda.synchronize()
        lap["normalise+encode"] = time.perf_counter() - t
        return time.perf_counter() - t0, lap, tuple(mu.shape)

    run(warm)                                           # first-call costs of the PROCESS (code objects, streams) stay out of the figure
    torch.cuda.empty_cache()                            # ... but not the allocations: the first pass below starts without cached blocks
    passes = [run(fq) for _ in range(2)]
    total, lap, shape = passes[0]                       # pangaea.py extracts features ONCE per data set: the first pass is the figure
    for f in (fq, warm):
        os.remove(f)
    os.rmdir(tmp)
    threads = min(32, len(os.sched_getaffinity(0)))
    return {"value": n / total, "unit": "pairs/s", "pairs": n, "fastq_bytes": size, "host_threads": threads,
            "first_pass": n / passes[0][0], "best_of_two": n / min(p[0] for p in passes),
            "seconds": {k: round(v, 4) for k, v in lap.items()}, "mu_shape": list(shape),
            "what": "plain interleaved FASTQ file (page cache) -> ingest with the H2D copy of finished pieces under the parse (the pipeline's scratch allocated by a helper "
                    "thread meanwhile) -> table sizing + allocation + plan + count/lookups -> rows -> normalise -> encode, one GPU; value = first_pass = the FIRST pass over "
                    "the file with an empty allocator cache (what one Feature call costs), best_of_two = the faster of two passes"}


def spawn_ranks(n: int) -> int:
    """``python bench.py --gpus N`` without a launcher: start N rank processes of this same command (one per GPU, RCCL
    rendezvous on 127.0.0.1) and wait for them.  The parent never touches the GPU (nothing here initialises HIP), so
    the children are ordinary fresh processes; rank 0's JSON line passes through on stdout."""
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    try:
        pending = set(range(n))
        while pending:
            for r in sorted(pending):
                code = procs[r].poll()
                if code is None:
                    continue
                pending.discard(r)
                if code != 0 and rc == 0:
                    rc = code
                    for o in pending:               # one rank failed: the others would wait in a collective for ever
                        procs[o].terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and args.rehearse_dist <= 1:
        raise SystemExit(spawn_ranks(args.gpus))
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the feature path has no CPU fallback")
    local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    multi = world > 1 or args.rehearse_dist > 1
    if args.rehearse_dist > 1 and world == 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29599")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        if args.rehearse_dist >= 4:
            from pangaea_amd import dist as _pd
            _pd.OWNER_MIN_WORLD = 1          # the owner-partitioned exchange (all-to-all + all-gather), as 4+ ranks run it
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    from pangaea_amd import dist as pdist
    from pangaea_amd import kmer, runtime, synth
    from pangaea_amd.data import Data
    from pangaea_amd.models.VAENET import VAENET

    # once per PROCESS, as Feature does when a call begins (under its ingest): the GEMM library's initialisation, on a helper thread
    runtime.warm_blas(dev)

    n_bc = args.barcodes or max(1, args.pairs // 200)
    cfg = synth.SynthConfig(n_pairs=args.pairs, n_barcodes=n_bc, read_len=READ_LEN, seed=2022, first_pair=rank * args.pairs)
    stream = synth.generate(cfg, device=dev, chunk_pairs=1 << 17, with_names=False)
    t_s = time.perf_counter()
    rows = stream.rows(MIN_LEN)
    plan = kmer.Plan(rows, dev)
    torch.cuda.synchronize()
    rows_ms = (time.perf_counter() - t_s) * 1e3
    # table sized from HyperLogLog sketches, outside the timed region: the elementwise maximum of the ranks' sketches is the
    # sketch of the union, so every rank allocates the same table (geometry of the union) at load <= 0.6
    # (what a NEW data set costs before its first step is reported as `setup_ms`: the device-resident figure leaves it out)
    setup = {}
    torch.cuda.synchronize(); t_s = time.perf_counter()
    regs = kmer.distinct_sketch(stream, K_ABD)
    local_distinct = kmer.sketch_estimate(regs)
    setup["distinct_sketch"] = (time.perf_counter() - t_s) * 1e3
    setup["rows+plan_segments"] = rows_ms
    if multi:
        union = regs if args.backend == "nccl" else regs.cpu()
        dist.all_reduce(union, op=dist.ReduceOp.MAX)
        regs = union
    for r in range(1, args.rehearse_dist if world == 1 else 0):           # rehearsal: the sketches of the other shards
        other = synth.generate(synth.SynthConfig(n_pairs=args.pairs, n_barcodes=n_bc, read_len=READ_LEN, seed=2022, first_pair=r * args.pairs),
                               device=dev, chunk_pairs=1 << 17, with_names=False)
        regs = torch.maximum(regs, kmer.distinct_sketch(other, K_ABD).to(regs.device))
        del other
    hint = max(1 << 14, int(1.05 * kmer.sketch_estimate(regs)))
    fused = not multi and not args.no_fuse
    import math
    mini = fused and not args.no_mini and kmer.KmerTable.mini_applies(K_ABD, max(10, math.ceil(math.log2(max(1024, int(hint / args.load))))))
    torch.cuda.synchronize(); t_s = time.perf_counter()
    # N > 1 ranks: the super-k-mer pipeline on every rank's own reads, entries to bucket owners, bins back (dist.MiniSharded);
    # --no-mini: round 1's key-partitioned pipeline with the replicated table
    ms = None
    if multi and not args.no_mini:
        loc = torch.tensor([int(1.1 * local_distinct)], dtype=torch.int64, device=dev if args.backend == "nccl" else "cpu")
        if world > 1:
            dist.all_reduce(loc, op=dist.ReduceOp.MAX)
        log2_u, lb_u, lb_l = pdist.MiniSharded.geometry(hint, int(loc.item()), union_load=args.load)
        if log2_u - lb_u <= 16:
            ms = pdist.MiniSharded(K_ABD, dev, log2_u, lb_l, WINDOW, VSIZE, union_log2_bucket=lb_u)
    table = ms.union if ms is not None else kmer.KmerTable.alloc(K_ABD, dev, "mini" if mini else "hash", distinct_hint=hint, load=args.load)
    torch.cuda.synchronize()
    setup["table_alloc"] = (time.perf_counter() - t_s) * 1e3
    # N > 1: a rank's own keys are 2^g times sparser than the union and are counted in deferred form (entries + fills for
    # the exchange; the rank's own sparse table is never written)
    defer = pdist.deferred_group_for(table, int(1.1 * local_distinct)) if multi and ms is None and not args.no_defer else None
    tnf = torch.zeros((len(rows), kmer.tnf_ncols(K_TNF)), dtype=torch.int32, device=dev)
    abd = torch.zeros((len(rows), VSIZE), dtype=torch.int32, device=dev)
    torch.manual_seed(2021)
    vae = VAENET(VSIZE, tnf.shape[1], 32, 30, 1, True, 1, 0.005, 0.2, 0.1, 0.015, 0.0001)
    vae.network.eval()
    names = np.array(rows.names, dtype=object)

    k2 = "kmer_count+lookup" if fused else "kmer_count"
    alg = ALG_BYTES_FUSED if fused else ALG_BYTES
    ev = {k: [] for k in ((k2, "exchange", "features") if multi else (k2, "features"))}

    side = torch.cuda.Stream(device=dev)

    tnf_side = torch.cuda.Stream(device=dev)

    def tnf_beside(cur):
        """K1 (TNF rows) depends on the reads alone and could run on a stream of its own beside the table kernels (PG_TNF_BESIDE=1).
        Measured on one GPU: the first scatter pass, which is bound by VALU issue, slows down by more than K1 takes -- stage + 1.8 ms,
        features - 0.8 ms, step 35.1 instead of 34.1 ms -- so the default keeps K1 behind the row histograms."""
        tnf_side.wait_stream(cur)
        with torch.cuda.stream(tnf_side):
            kmer.features(stream, plan, k_tnf=K_TNF, table=None, out_tnf=tnf)

    beside = os.environ.get("PG_TNF_BESIDE", "0") not in ("", "0")

    def step_sharded(timed: bool):
        """N > 1 ranks, super-k-mer form: count half | entries to owners, merged bins back | lookup half + rows + TNF"""
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        cur = torch.cuda.current_stream(dev)
        if args.plan != "once":
            ms.local._mini_plan = None
        ms.count_half(stream, plan)
        e[1].record()
        # work that needs nothing from the other ranks goes beside the exchange, whose collectives and host-side sizing leave the GPU
        # idle in between: the TNF rows (they depend on the reads alone) and the next batch's partition plan
        in_gaps = os.environ.get("PG_EXCHANGE_GAPS", "1") not in ("", "0")
        if in_gaps:
            tnf_beside(cur)
            if args.plan == "ahead":
                ms.local.prefetch_plan(stream, plan, side)
        ms.exchange()
        e[2].record()
        if args.plan == "ahead" and not in_gaps:      # the next batch's plan: beside the lookup half (LDS-bound) and the row histograms
            ms.local.prefetch_plan(stream, plan, side)
        ms.lookup_half()
        kmer.features(stream, plan, k_tnf=None if in_gaps else K_TNF, table=ms.local, window=WINDOW, vsize=VSIZE, out_tnf=None if in_gaps else tnf, out_abd=abd)
        if in_gaps:
            cur.wait_stream(tnf_side)
        e[3].record()
        mu = vae.encode(Data(names, abd, tnf, device=dev))
        if timed:
            ev[k2].append((e[0], e[1]))
            ev["exchange"].append((e[1], e[2]))
            ev["features"].append((e[2], e[3]))
        return mu

    def step(timed: bool):
        if ms is not None:
            return step_sharded(timed)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        cur = torch.cuda.current_stream(dev)
        if beside:
            tnf_beside(cur)
        table.reset()                   # bucketed tables are overwritten slice by slice: no 4 GB clear
        if mini and args.plan != "once":
            table._mini_plan = None         # every step plans its batch: in front of the count, or ahead (prefetched by the step before)

        # one GPU: the lookup pass of the abundance rows rides inside the counting kernel (same table, same matrices)
        table.count(stream, check=False, rows=plan, deferred_group=defer if defer is not None and table.can_defer(stream.n_words) else None,
                    emit=(WINDOW, VSIZE) if fused else None)
        e[1].record()
        if mini and args.plan == "ahead":
            # the next batch's plan, on a side stream behind this batch's count: it runs beside the row histograms and the encode
            # (2.3 of its 2.7 ms stay visible).  PG_PLAN_WHERE=second-pass starts it behind the FIRST scatter pass instead, beside
            # the memory-bound second pass (1.6 ms visible: the step is 0.7 ms shorter, but the roofline stage below then carries
            # another batch's plan in its time -- not the default for that reason); =first-pass: beside everything (all visible)
            where = os.environ.get("PG_PLAN_WHERE", "")
            table.prefetch_plan(stream, plan, side, after="first-pass" if where == "second-pass" else e[0] if where == "first-pass" else None)
        if world > 1:
            pdist.exchange_table(table, check=False)
        elif multi:
            pdist._exchange_bucketed(table)         # rehearsal: the same launches and collectives in a one-rank group
        e[2].record()
        kmer.features(stream, plan, k_tnf=None if beside else K_TNF, table=table, window=WINDOW, vsize=VSIZE, out_tnf=None if beside else tnf, out_abd=abd)
        if beside:
            cur.wait_stream(tnf_side)
        e[3].record()
        d = Data(names, abd, tnf, device=dev)
        mu = vae.encode(d)
        if timed:
            ev[k2].append((e[0], e[1]))
            ev["features"].append((e[2], e[3]))
            if multi:
                ev["exchange"].append((e[1], e[2]))
        return mu

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(args.warmup):
        if i == 0:
            torch.cuda.synchronize(); t_s = time.perf_counter()
        mu = step(False)
        if i == 0:                      # the first pass over a data set: workspaces, code objects and -- super-k-mer pipeline -- the first plan
            torch.cuda.synchronize()
            setup["first_step_incl_allocations"] = (time.perf_counter() - t_s) * 1e3
    fence()
    ms.check_status() if ms is not None else table.check_status()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        mu = step(True)
    fence()
    elapsed = time.perf_counter() - t0
    ms.check_status() if ms is not None else table.check_status()
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    assert tuple(mu.shape) == (len(rows), 32) and bool(torch.isfinite(mu).all())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, mu, tnf, abd)

    kern_ms = {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in ev.items()}
    table_load = table.occupancy() if table.kind == "hash" else None
    dominant = max((k for k in kern_ms if k != "exchange"), key=kern_ms.get)
    achieved = alg[dominant] * args.pairs / (kern_ms[dominant] * 1e-3) / 1e9
    traffic = traffic_tag = None
    tpath = os.path.join(ROOT, "profiles", "traffic.json")        # per-launch HBM bytes from rocprofv3 --pmc passes
    if os.path.exists(tpath):
        with open(tpath) as f:
            tj = json.load(f)
        if tj.get("pairs") == args.pairs and tj.get("pipeline", "key") == ("mini" if mini else "key"):
            traffic = tj.get("kernels", {}).get(dominant)
            traffic_tag = tj.get("tag")             # (which build the PMC passes were collected for: profiles/README.md)

    if rank == 0:
        out = {
            "metric": "barcoded read-pairs/sec through feature+VAE-encode",
            "value": world * args.pairs * args.steps / elapsed,
            "unit": "pairs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u64",
            "data": "synthetic",
            "config": {"workload": f"synthetic {args.pairs} x 150 bp read pairs and {n_bc} barcodes per GPU, k=21 hash table "
                                   f"(2^{table.log2_slots} slots), TNF k=4 + abundance V=400 W=10, L1-normalise, VAE 536-512-512-32 encode",
                       "pairs_per_gpu": args.pairs, "barcodes_per_gpu": n_bc, "rows_per_gpu": len(rows),
                       "parallelism": ((f"run-sharded x{world}, super-k-mer count half per rank, entries to bucket owners (all-to-all, 8 B per distinct k-mer), "
                                        f"merged bins back (all-to-all, 2 B), lookup half per rank ({args.backend})") if world > 1 and ms is not None
                                       else f"run-sharded x{world}, deferred count, " + ("owner-partitioned table exchange (all-to-all + all-gather of merged ranges, 6-byte entries)"
                                                                                    if world >= 4 else "range-wise table all-gather (6-byte entries) overlapped with LDS rebuilds")
                                       + f" ({args.backend})" if world > 1
                                       else f"REHEARSAL of the {args.rehearse_dist}-rank path on one GPU (one-rank RCCL group)" if multi else "single GPU"),
                       "pipeline": ("super-k-mers by minimizer bucket (12-byte records, LDS counting per bucket; lookups of the provisional words once the owners' bins are back)"
                                    if ms is not None else
                                    "super-k-mers by minimizer bucket (12-byte records, LDS counting + lookups per bucket)" if mini
                                    else "k-mer occurrences by key (8-byte records, LDS counting" + (" + lookups" if fused else "") + " per bucket)"),
                       "partition_plan": ({"ahead": "computed in every step for the next batch, on a side stream under the row histograms and the encode",
                                            "in-step": "computed in every step, in front of the count",
                                            "once": "computed ONCE before the timed steps (comparison figure: only valid because the bench repeats one batch)"}[args.plan]
                                          if mini else "bucket histogram inside the step"),
                       "records_per_pair": (ms.local.plan_counts()[0] / args.pairs if ms is not None and ms.local._mini_plan else
                                            table.plan_counts()[0] / args.pairs if mini and table._mini_plan else 260.0),
                       "exchange_bytes_per_rank": ({"sent": ms.bytes_sent, "received": ms.bytes_received} if ms is not None else None),
                       "local_bucket_slots": (1 << ms.local.log2_bucket if ms is not None else None),
                       "tnf_rows": ("on a stream of their own beside the table kernels" if beside else "behind the row histograms"),
                       "input": "packed reads resident in HBM", "table_load": table_load,
                       "table_buckets": table.n_buckets, "bucket_slots": 1 << table.log2_bucket if table.log2_bucket else None},
            "kernel_ms": kern_ms,
            "roofline": {"bound": "hbm", "kernel": dominant, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_tag": traffic_tag,
                         "alg_bytes_per_pair": alg[dominant]},
            "setup_ms": {k: round(v, 2) for k, v in setup.items()},
        }
        if args.full and world == 1 and args.e2e_pairs != 0 and not args.rehearse_dist:
            try:
                del table                       # (the leg builds its own: two 8.6 GB tables and their workspaces need not coexist)
                torch.cuda.empty_cache()
                out["e2e"] = e2e_leg(stream, cfg, args.pairs if args.e2e_pairs < 0 else min(args.e2e_pairs, args.pairs), vae, dev)
            except Exception as e:          # reporting only
                out["e2e"] = {"value": None, "unit": "pairs/s", "what": f"failed: {e!r}"}
        if args.full and world == 1 and not args.no_cpu_baseline:
            state = {k: v.detach().cpu().numpy() for k, v in vae.network.state_dict().items()}
            try:
                out["cpu_baseline"] = cpu_baseline(stream, cfg, min(args.cpu_sample, args.pairs), state)
            except Exception as e:          # the baseline is reporting only; never lose the GPU line over it
                out["cpu_baseline"] = {"value": None, "unit": "pairs/s", "cores": 0, "kind": "port", "sample": f"failed: {e!r}"}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
    if multi:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
