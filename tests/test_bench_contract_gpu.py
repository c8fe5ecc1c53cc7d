"""bench.py's one JSON line carries every key the driver's contract names (small workload, one GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from .conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("extra", [[], ["--no-mini"], ["--no-fuse"], ["--rehearse-dist", "4"]])
def test_bench_line_honours_the_contract(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--pairs", "200000", "--steps", "2", "--warmup", "1", "--full", "--cpu-sample", "2000"] + extra
    if extra:
        cmd.append("--no-cpu-baseline")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline"):
        assert key in j, key
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1 and j["higher_is_better"] is True and j["scaling"] == "weak"
    assert j["unit"] == "pairs/s" and j["vs_baseline"] is None and j["data"] == "synthetic" and j["dtype"] == "u64"
    assert abs(j["value"] - 200000 * 2 / (j["ms_per_step"] * 2e-3)) < 1e-6 * j["value"]
    assert "workload" in j["config"] and "model" not in j["config"]
    r = j["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert "traffic" in r and "traffic_tag" in r and r["kernel"] in j["kernel_ms"]
    assert {"distinct_sketch", "table_alloc", "rows+plan_segments", "first_step_incl_allocations"} <= set(j["setup_ms"])     # what `value` leaves out
    if not extra:
        c = j["cpu_baseline"]
        assert c["unit"] == "pairs/s" and c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
        assert "super-k-mer" in j["config"]["pipeline"]
    if extra in ([], ["--no-mini"]):
        e = j["e2e"]                                    # the FASTQ -> mu leg, reported beside the device-resident value
        assert e["unit"] == "pairs/s" and e["value"] > 0 and e["pairs"] == 200000 and e["host_threads"] >= 1
        # shape only: which of two timings of a 200 k-pair toy workload wins is data, not a contract (round 3's driver box had it the other way)
        assert set(e["seconds"]) == {"ingest+h2d", "table+rows", "normalise+encode"}
        assert e["first_pass"] == e["value"] and 0 < e["value"] <= e["best_of_two"] * 1.0000001
    if extra == ["--rehearse-dist", "4"]:
        p = j["config"]["pipeline"]
        assert "exchange" in j["kernel_ms"] and ("lookup half" in p or "lookups of the provisional words" in p)


def test_plain_bench_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """without --full the line leaves out the CPU baseline and the FASTQ leg; --dump-outputs writes the last timed step's mu, TNF and
    abundance rows (float32 / float64, under 64 MB), and two runs with the same arguments write the same rows"""
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--pairs", "200000", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        j = json.loads(lines[0])
        assert j["steps"] == 3 and j["warmup"] == 1 and "cpu_baseline" not in j and "e2e" not in j
        assert abs(j["value"] - 200000 * 3 / (j["ms_per_step"] * 3e-3)) < 1e-6 * j["value"]
        files = sorted(os.listdir(d))
        assert files == ["abd.npy", "mu.npy", "tnf.npy"]
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        a = {f[:-4]: np.load(d / f) for f in files}
        n = j["config"]["rows_per_gpu"]                 # 1 000 rows: every one of them is dumped
        assert a["mu"].dtype == np.float32 and a["mu"].shape == (n, 32) and np.isfinite(a["mu"]).all()
        assert a["tnf"].dtype == np.float64 and a["tnf"].shape == (n, 136) and a["abd"].dtype == np.float64 and a["abd"].shape == (n, 400)
        assert a["tnf"].sum() > 0 and a["abd"].sum() > 0
        dumps.append(a)
    assert np.array_equal(dumps[0]["tnf"], dumps[1]["tnf"]) and np.array_equal(dumps[0]["abd"], dumps[1]["abd"])
    np.testing.assert_allclose(dumps[0]["mu"], dumps[1]["mu"], rtol=1e-5, atol=1e-6)


def test_bench_starts_its_own_ranks():
    """``python bench.py --gpus 2`` with no launcher around it: two rank processes, one JSON line with n_gpus 2 (gloo here: the
    two ranks share the one GPU of the box, which RCCL does not allow)"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--pairs", "200000", "--steps", "1", "--warmup", "1",
           "--no-cpu-baseline"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and "exchange" in j["kernel_ms"]
    assert abs(j["value"] - 2 * 200000 / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
