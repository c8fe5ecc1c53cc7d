#!/usr/bin/env python3
"""time the silhouette by which step 3 picks the number of clusters (pangaea_amd/clustering.py: dist_sums, choose_clusters;
csrc/cluster.hip: pg_cluster_dist_sums) on one GPU, with HIP events, after warm-up, repeated, with the spread.

Latents: the 1 M synthetic rows of tools/bench_train_cluster.py (count matrices around 30 prototype profiles, one epoch of
VAE training, the encode), dim 32.  Shapes:
  (a) N = 50 000 (BASELINE config 2's rows), exact (M = N), k = 40
  (b) N = 1 000 000, M = 16 384 sampled query rows, k = 40 and k = 100
  (c) the whole default choose_clusters (range 4..100 step 3, patience 7, 16 384 sampled rows, n_init 5) on the 1 M rows
Per shape: pg_cluster_dist_sums alone (rows sorted beforehand), dist_sums all in (sort + gather + kernel), the torch form of
dist_sums (PG_SILHOUETTE_KERNEL=0: tiles of float64 torch.cdist times a one-hot matrix) and a device copy of the reference
rows, the least any pass over them costs.  Pairs per second stand beside the rate the kernel's instruction budget implies.

    python tools/time_silhouette.py [--rows 1000000] [--out profiles/time_silhouette.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pangaea_amd import _lib, clustering  # noqa: E402

# the dim == 32 kernel per (query row, reference row), in vector instructions of one lane: 32 subtracts and 32 fused multiply-adds,
# the square root as the compiler expands it for the full float32 range (16 instructions, v_sqrt_f32 itself counted as 8: a
# quarter of the plain rate), the add into the float32 partial sum, and 1/8 of the conversion and the float64 add that fold it.
# The rate: the float32 vector peak of 64 FLOP per clock and SIMD = 32 lanes of one fused multiply-add per clock -- DESIGN.md
SLOTS_PER_PAIR = 64 + 15 + 8 + 1 + 0.5
LANES_PER_CLOCK = 256 * 4 * 32          # 256 CUs x 4 SIMDs x 32 lanes
CLOCK_HZ = 2.4e9
BUDGET_PAIRS_PER_S = LANES_PER_CLOCK * CLOCK_HZ / SLOTS_PER_PAIR


def events_ms(fn, warmup, repeats):
    """the times of ``repeats`` calls in ms, each between two events, after ``warmup`` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def summary(ms, pairs=None):
    ms = sorted(ms)
    d = {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "repeats": len(ms)}
    if pairs is not None:
        d["pairs_per_s"] = float(f"{pairs / (d['median_ms'] * 1e-3):.4g}")
        d["share_of_budget_rate"] = round(d["pairs_per_s"] / BUDGET_PAIRS_PER_S, 3)
    return d


def synthetic_latents(rows, dev):
    """tools/bench_train_cluster.py's rows: counts around 30 prototype profiles -> Data -> one epoch of training -> latent"""
    from pangaea_amd.data import Data
    from pangaea_amd.loader import shuffled_batches, weighted_batches
    from pangaea_amd.models.VAENET import VAENET
    clusters, batch = 30, 2048
    np.random.seed(2021)
    torch.manual_seed(2021)
    g = torch.Generator(device=dev).manual_seed(1)
    proto_a = torch.rand((clusters, 400), generator=g, device=dev) ** 4
    proto_t = torch.rand((clusters, 136), generator=g, device=dev) + 0.2
    which = torch.randint(0, clusters, (rows,), generator=g, device=dev)
    abd = torch.poisson(proto_a[which] * 300, generator=g).to(torch.int32)
    tnf = torch.poisson(proto_t[which] * 400, generator=g).to(torch.int32)
    data = Data(np.array([f"bc{i}" for i in range(rows)], dtype=object), abd, tnf, device=dev)
    train = weighted_batches(data, batch)
    test = weighted_batches(data, batch, num_samples=min(int(rows * 0.7), 1_000_000), replacement=False)
    orig = shuffled_batches(data, batch)
    vae = VAENET(400, 136, 32, clusters, 1, True, 1, 0.005, 0.2, 0.1, 0.015, 0.0001)
    tmp = tempfile.mkdtemp(prefix="pg_sil_")
    vae.train(train, test, orig, tmp, patience=10_000)
    latent = np.load(os.path.join(tmp, "latent.npz"))["arr_0"]
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
    return latent.astype(np.float32)


def time_shape(x, rows, k, dev, repeats):
    """one (N, M, k), labels from five Lloyd iterations from k random rows: the kernel alone, dist_sums all in, the torch form
    (checked against the kernel at this very size), a copy of the rows"""
    L = _lib.load()
    n, m = x.shape[0], (x.shape[0] if rows is None else len(rows))
    g = torch.Generator(device=dev).manual_seed(k)
    labels = clustering.lloyd(x, x[torch.randperm(n, generator=g, device=dev)[:k]], max_iter=5)[0]
    q = x if rows is None else x[torch.from_numpy(rows).to(dev)]
    order = torch.argsort(labels, stable=True)
    xs = x[order].contiguous()
    seg = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    seg[1:] = torch.cumsum(torch.bincount(labels, minlength=k), 0)
    need = _lib.check(L.pg_cluster_dist_sums_workspace_bytes(m, n, k, 0))
    work = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    out = torch.empty((m, k), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        _lib.check(L.pg_cluster_dist_sums(q.data_ptr(), m, xs.data_ptr(), n, 32, seg.data_ptr(), k, 0, out.data_ptr(), work.data_ptr(), need, stream))

    res = {"N": n, "M": m, "k": k, "pairs": m * n, "n_splits": need // (m * k * 8) if need else 1}
    res["kernel"] = summary(events_ms(kernel, 2, repeats), m * n)
    res["dist_sums_all_in"] = summary(events_ms(lambda: clustering.dist_sums(q, x, labels, k), 2, repeats), m * n)
    os.environ["PG_SILHOUETTE_KERNEL"] = "0"
    try:
        clustering.dist_sums(q[:256], x, labels, k)                # (warm-up on a slice: the full call takes seconds at 1 M rows)
        kept = []
        res["torch_form"] = summary(events_ms(lambda: kept.append(clustering.dist_sums(q, x, labels, k)), 0, 2), m * n)
        torch_sums = kept[-1]
    finally:
        os.environ.pop("PG_SILHOUETTE_KERNEL", None)
    kernel_sums = clustering.dist_sums(q, x, labels, k)
    some = torch_sums > 0
    res["kernel_vs_torch_form_max_rel"] = float(((kernel_sums - torch_sums).abs()[some] / torch_sums[some]).max())
    res["kernel_zero_where_torch_form_zero"] = bool((kernel_sums[~some] == 0).all())
    dst = torch.empty_like(xs)
    res["copy_of_reference_rows"] = summary(events_ms(lambda: dst.copy_(xs), 2, repeats))
    res["torch_form_over_kernel"] = round(res["torch_form"]["median_ms"] / res["kernel"]["median_ms"], 2)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_silhouette.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_silhouette.py needs a GPU"
    dev = torch.device("cuda:0")
    t = time.perf_counter()
    latent = synthetic_latents(args.rows, dev)
    print(f"latents {latent.shape} in {time.perf_counter() - t:.1f} s", flush=True)
    x = torch.from_numpy(latent).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "latent_rows": args.rows, "dim": 32,
              "budget": {"issue_slots_per_pair": SLOTS_PER_PAIR, "lanes_per_clock": LANES_PER_CLOCK, "clock_hz": CLOCK_HZ,
                         "pairs_per_s": float(f"{BUDGET_PAIRS_PER_S:.4g}")},
              "shapes": []}
    np.random.seed(2021)
    small = min(50_000, args.rows)
    result["shapes"].append(dict(time_shape(x[:small].contiguous(), None, 40, dev, args.repeats), name="a: exact, 50 000 rows"))
    rows = clustering._sample_rows(args.rows, 16384, 0)
    for k in (40, 100):
        result["shapes"].append(dict(time_shape(x, rows, k, dev, args.repeats), name=f"b: 16 384 of 1 M rows, k = {k}"))
    sweeps = []
    for _ in range(3):
        np.random.seed(2021)
        torch.cuda.synchronize()
        t = time.perf_counter()
        best, table = clustering.choose_clusters(x)
        torch.cuda.synchronize()
        sweeps.append(time.perf_counter() - t)
        print(f"choose_clusters: {sweeps[-1]:.2f} s, best k = {best}, {len(table)} k visited", flush=True)
    result["choose_clusters"] = {"name": "c: default sweep on the 1 M rows", "seconds": [round(s, 3) for s in sweeps], "best_k": best,
                                 "visited": len(table), "table": [[k, round(s, 6), round(i, 3), c] for k, s, i, c in table]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
