"""bench.py --dump-outputs on the host: which rows a dump keeps, its file types and its size bound (the GPU run is in
test_bench_contract_gpu.py)."""
import os

import numpy as np
import torch

import bench


def test_dump_rows_are_all_rows_or_a_fixed_sorted_sample():
    assert np.array_equal(bench.dump_rows(1000, 8192), np.arange(1000))
    s = bench.dump_rows(500_000, 8192)
    assert len(s) == 8192 and len(np.unique(s)) == 8192 and np.all(np.diff(s) > 0) and s[-1] < 500_000
    assert np.array_equal(s, bench.dump_rows(500_000, 8192))


def test_dump_outputs_keeps_the_sampled_rows_exactly_and_under_64_mb(tmp_path):
    n = 200_000                                     # 1 000 pairs per row at the default 200: a 200 M-pair batch
    g = torch.Generator().manual_seed(7)
    mu = torch.randn((n, 32), generator=g)
    tnf = torch.randint(0, 1 << 20, (n, 136), dtype=torch.int32, generator=g)
    abd = torch.randint(0, 1 << 30, (n, 400), dtype=torch.int32, generator=g)
    bench.dump_outputs(str(tmp_path), mu, tnf, abd)
    files = sorted(os.listdir(tmp_path))
    assert files == ["abd.npy", "mu.npy", "tnf.npy"]
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20
    m, t, a = (np.load(tmp_path / f"{k}.npy") for k in ("mu", "tnf", "abd"))
    assert m.dtype == np.float32 and t.dtype == np.float64 and a.dtype == np.float64
    rm, rf = bench.dump_rows(n, bench.DUMP_MU_ROWS), bench.dump_rows(n, bench.DUMP_FEATURE_ROWS)
    assert np.array_equal(m, mu.numpy()[rm])
    assert np.array_equal(t, tnf.numpy()[rf].astype(np.float64)) and np.array_equal(a, abd.numpy()[rf].astype(np.float64))
