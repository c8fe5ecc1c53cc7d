"""The super-k-mer form on N > 1 ranks (dist.MiniSharded) for MASKED input: bases below the quality threshold (the table leaves
them out, jellyfish --min-qual-char=?, feature.py:76-83; the rows do not look at qualities) and soft-masked reads counted with
lower-case bases (the rows reset on them).  Ranks share cuda:0 over gloo, as in test_dist_gloo.py.  A k-mer that only a row sees
takes a local slot with count 0 and is looked up at its owner: bin of what the other ranks counted, or none (count_kmer.cpp:87)."""
import gzip
import os
import socket

import numpy as np
import pandas as pd
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import oracle
from pangaea_amd import _lib
from pangaea_amd import dist as pdist
from pangaea_amd import feature, kmer, synth
from pangaea_amd.reads import ReadStream

from .conftest import GOLDEN, ROOT

K, W, V = 21, 10, 400


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(fn, world, *args):
    mp.spawn(fn, args=(world, _free_port()) + args, nprocs=world, join=True)


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _plane(mask: np.ndarray, n_words: int) -> torch.Tensor:
    """a per-character boolean mask as a validity plane (bit j of word w = character 32 w + j)"""
    m = np.zeros(n_words * 32, dtype=np.uint64)
    m[:mask.size] = mask
    bits = (m.reshape(n_words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return torch.from_numpy(bits.view(np.int32).copy())


def _bits(plane: torch.Tensor, n_chars: int) -> np.ndarray:
    v = plane.cpu().numpy().view(np.uint32).astype(np.uint64)
    return ((v[:, None] >> np.arange(32, dtype=np.uint64)) & 1).reshape(-1)[:n_chars].astype(bool)


def _mini_cfg():
    return synth.SynthConfig(n_pairs=24_000, n_barcodes=150, n_genomes=3, genome_len=40_000, fragment=10_000, sub_rate=0.01, n_rate=0.05, seed=321)


def _stream(case: str, k: int = K) -> ReadStream:
    """the whole input of a case, on the host (every process builds the same one)"""
    rng = np.random.RandomState(7)
    if case in ("qual", "both"):
        s = synth.generate(_mini_cfg())
        valid = _bits(s.valid, s.n_chars)
        lower = None
        if case == "both":                         # soft-masked bases: out of `valid`, into `valid_lower`
            lower = valid & (rng.rand(s.n_chars) < 0.03)
            valid = valid & ~lower
            s.valid = _plane(valid, s.n_words)
            s.valid_lower = _plane(lower, s.n_words)
        # about 8 % low-quality bases, denser towards the ends of the 150-character reads
        pos = np.arange(s.n_chars) % 151
        p = 0.04 + 0.12 * (np.minimum(pos, 150 - pos) < 20)
        base = valid if lower is None else valid | lower
        s.valid_lowq = _plane(base & (rng.rand(s.n_chars) < p), s.n_words)
        return s
    if case in ("polya", "polya0"):
        # runs of A (and of T: the same canonical k-mer, code 0) of 10/7 k and 25/21 k (k = 21: 30 and 25) with a low-quality base in
        # the middle, so that no clean stretch reaches k, a few A's of the random text beside it included (test_masked_host.py checks
        # that): every all-A k-mer there is row-only.  "polya": the first runs also hold clean A runs, so some rank counts the all-A
        # k-mer; "polya0": nobody does.
        a, c = k + 3 * k // 7, k + 4 * k // 21
        rnd = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))
        runs, lowq = [], []
        for i in range(60):
            body = rnd(120) + b"A" * a + rnd(80) + b"T" * a + rnd(60) + b"A" * c + rnd(40)
            marks = [120 + a // 2, 120 + a + 80 + a // 2 - 1, 120 + a + 80 + a + 60 + c // 2]
            if case == "polya" and i < 6:
                body += b"A" * max(70, k + 49)
            body += b"N"
            runs.append((f"bc{i:03d}", body))
            lowq.append(marks)
        s = ReadStream.from_runs(runs)
        mask = np.zeros(s.n_chars, dtype=bool)
        for i, marks in enumerate(lowq):
            mask[int(s.run_off[i]) + np.array(marks)] = True
        s.valid_lowq = _plane(mask, s.n_words)
        return s
    if case == "sat":
        # 3.1 M copies of the all-A 21-mer (A and T runs) on EVERY rank, a low-quality base every 1000 characters: some 33 k copies
        # per rank are row-only, the counted ones saturate every rank's part
        s = ReadStream.from_runs([("a", b"A" * 1_600_000 + b"N" + b"T" * 1_500_040 + b"N"), ("b", b"ACG" * 30_000 + b"N")])
        mask = np.zeros(s.n_chars, dtype=bool)
        mask[500:3_100_000:1000] = True
        mask &= _bits(s.valid, s.n_chars)
        s.valid_lowq = _plane(mask, s.n_words)
        return s
    raise ValueError(case)


def _lc(case):
    return case == "both"


def _min_len(case):
    return 0 if case == "sat" else 100 if case.startswith("polya") else 2000


def _worker(rank, world, port, outdir, case, pieces, k=K, window=W, vsize=V):
    _init(rank, world, port)
    try:
        s = _stream(case, k)
        part = (s if case == "sat" else pdist.shard_stream(s, rank, world)).to("cuda:0")
        assert kmer.KmerTable.half_masked(part, _lc(case))
        if pieces:
            os.environ["PANGAEA_MINI_PIECE_WORDS"] = str(part.n_words // pieces + 256)
        rows = part.rows(_min_len(case))
        plan = kmer.Plan(rows, "cuda:0")
        assert feature._sharded_mini_applies(part, plan, k, window, vsize, _lc(case))
        tnf, abd, ms = pdist.features_sharded_mini(part, plan, k, 4, window, vsize, lowercase_is_base=_lc(case))
        assert isinstance(ms, pdist.MiniSharded) and ms.masked and ms.local.k == ms.union.k == k
        assert ms.local.n_buckets == ms.union.n_buckets >= 512
        if pieces:
            assert ms.pieces >= pieces
        c, n = ms.owned_items()
        np.savez(os.path.join(outdir, f"m{rank}.npz"), c=c, n=n, tnf=tnf.cpu().numpy(), abd=abd.cpu().numpy(), names=np.array(rows.names))
        # counting again with the same object gives the same rows
        ms.count(part, plan)
        _, abd2 = kmer.features(part, plan, k_tnf=None, table=ms.local, window=window, vsize=vsize)
        assert torch.equal(abd2, abd)
    finally:
        dist.destroy_process_group()


def _has_poly_a(text: bytes, k: int) -> bool:
    """does the text hold an all-A k-mer window (as written, or as the reverse complement of T's)?"""
    return b"A" * k in text or b"T" * k in text


def _check(tmp_path, world, case, pieces=0, k=K, window=W, vsize=V, every_row=False):
    _spawn(_worker, world, str(tmp_path), case, pieces, k, window, vsize)
    parts = [np.load(str(tmp_path / f"m{r}.npz")) for r in range(world)]
    s = _stream(case, k).to("cuda:0")
    lc = _lc(case)
    table_text, strict_text = s.decode(plane=s.table_valid(lc)), s.decode()
    otab = oracle.Table(k, threads=4)
    for _ in range(world if case == "sat" else 1):
        otab.count(table_text)                             # ("sat": every rank holds a copy of the same reads)
    # the owners' ranges together are the oracle's table: counted k-mers only, none of count 0
    codes = np.concatenate([p["c"] for p in parts]); counts = np.concatenate([p["n"] for p in parts])
    order = np.argsort(codes)
    ocodes, ocounts = otab.items()
    assert counts.min() > 0
    assert np.array_equal(codes[order], ocodes) and np.array_equal(counts[order], np.minimum(ocounts, 1 << 21))
    rows = s.rows(_min_len(case))
    if case == "sat":
        assert counts.max() == 1 << 21 and codes[np.argmax(counts)] == 0
        for p in parts:
            for r in range(len(rows)):
                assert np.array_equal(p["abd"][r], oracle.abd_row(strict_text[rows.start[r]:rows.end[r]], k, otab, window, vsize))
        return
    names = [n for p in parts for n in p["names"].tolist()]
    assert names == list(rows.names)
    abd = np.concatenate([p["abd"] for p in parts]); tnf = np.concatenate([p["tnf"] for p in parts])
    # the one-process rows (a masked stream: table without rows, rows by lookups)
    plan = kmer.Plan(rows, "cuda:0")
    one = kmer.count_kmers(s, k, rows=plan, emit=(window, vsize), lowercase_is_base=lc)
    want_tnf, want_abd = kmer.features(s, plan, k_tnf=4, table=one, window=window, vsize=vsize)
    assert np.array_equal(abd, want_abd.cpu().numpy()) and np.array_equal(tnf, want_tnf.cpu().numpy())
    step = 1 if case.startswith("polya") or every_row else max(1, len(rows) // 8)
    for r in range(0, len(rows), step):
        assert np.array_equal(abd[r], oracle.abd_row(strict_text[rows.start[r]:rows.end[r]], k, otab, window, vsize))
    if case.startswith("polya"):                           # (not vacuous: rows do hold all-A k-mer windows, in the strict text)
        assert any(_has_poly_a(strict_text[rows.start[r]:rows.end[r]], k) for r in range(len(rows)))
    if case == "polya0":                                   # the all-A k-mer is in no table, and no row has a bin for it
        assert 0 not in set(ocodes.tolist())
    if case == "polya":
        assert 0 in set(ocodes.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_quality_masked_on_several_ranks(tmp_path, world):
    """a sparse low-quality plane inside `valid`: the masked count half on every rank, the masked owner merge; rows == the one-process
    rows == the oracle's (strict text, table of the table-plane text), owners' ranges == the oracle's table"""
    _check(tmp_path, world, "qual")


@pytest.mark.gpu
def test_quality_masked_with_one_count_workgroup_per_cu(tmp_path, monkeypatch):
    """PG_COUNT_BLOCK=1024: the masked count half in 1024-thread workgroups (what local buckets of 2^14 slots run)"""
    monkeypatch.setenv("PG_COUNT_BLOCK", "1024")
    _check(tmp_path, 2, "qual")


@pytest.mark.gpu
def test_soft_and_quality_masked_on_two_ranks(tmp_path):
    """lower-case bases counted (lowercase_is_base) and low-quality bases left out of the table: k-mers mixing the two kinds are
    neither counted nor looked up"""
    _check(tmp_path, 2, "both")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["polya", "polya0"])
def test_poly_a_with_low_quality_bases(tmp_path, case):
    """the all-A 21-mer has code 0: row-only, it must neither read as an empty slot nor leave an entry of 0 in the union"""
    _check(tmp_path, 2, case)


# (window, vsize) of the cases at k < 21, as in test_dist_gloo.py: k = 15 with the default flags
_KWV = {13: (1, 6), 14: (3, 64), 15: (10, 400), 16: (25, 512), 17: (2, 50), 18: (10, 400), 19: (1, 6), 20: (3, 64)}


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(_KWV))
def test_quality_masked_at_every_k(tmp_path, k):
    """13 <= k <= 20 on two ranks: the masked plan and first pass for every window length and both minimizer lengths, the masked
    count half and the masked owner merge in the instantiations for 4, 6 and 8 k-mers per record; every row against the oracle"""
    _check(tmp_path, 2, "qual", k=k, window=_KWV[k][0], vsize=_KWV[k][1], every_row=True)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [15, 18])
def test_soft_and_quality_masked_at_other_k(tmp_path, k):
    _check(tmp_path, 2, "both", k=k, window=_KWV[k][0], vsize=_KWV[k][1], every_row=True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["polya", "polya0"])
def test_poly_a_with_low_quality_bases_at_k15(tmp_path, case):
    """the all-A 15-mer (code 0, minimizers of 11): marked runs of 21 and 17, row-only as at k = 21"""
    _check(tmp_path, 2, case, k=15)


@pytest.mark.gpu
def test_masked_count_half_in_pieces_at_k15(tmp_path):
    _check(tmp_path, 2, "qual", pieces=3, k=15, every_row=True)


@pytest.mark.gpu
def test_saturation_with_row_only_copies(tmp_path):
    _check(tmp_path, 2, "sat")


@pytest.mark.gpu
def test_masked_count_half_in_pieces(tmp_path):
    """PANGAEA_MINI_PIECE_WORDS forces 3 pieces per rank: the row-only flags are cleared in every piece's kept meta words"""
    _check(tmp_path, 2, "qual", pieces=3)


def _golden_worker(rank, world, port, outdir):
    _init(rank, world, port)
    try:
        took = []
        orig = pdist.features_sharded_mini

        def spy(*a, **kw):
            r = orig(*a, **kw)
            took.append(r[2] is not None and r[2].masked)
            return r

        pdist.features_sharded_mini = spy
        out = {}
        r1, r2 = os.path.join(GOLDEN, "pairq_R1.fq"), os.path.join(GOLDEN, "pairq_R2.fq")
        for k in (15, 21):
            names, _, abd = feature.compute_features(r1, r2, k, 4, 1, 6, 100, device=torch.device("cuda", 0))
            out[f"pairq{k}"] = abd
            out[f"pairq{k}_names"] = np.array(names)
            names, _, abd = feature.compute_features(os.path.join(GOLDEN, "soft.fq"), None, k, 4, 1, 6, 100, device=torch.device("cuda", 0))
            out[f"soft{k}"] = abd
            out[f"soft{k}_names"] = np.array(names)
        assert took == [True] * 4, took
        np.savez(os.path.join(outdir, f"g{rank}.npz"), **out)
    finally:
        pdist.features_sharded_mini = orig
        dist.destroy_process_group()


@pytest.mark.gpu
def test_goldens_through_compute_features_on_two_ranks(tmp_path):
    """paired reads with low-quality bases and soft-masked reads, k = 15 and 21, under two gloo ranks: the gathered matrices are the
    reference's (the committed goldens), and both went through the masked super-k-mer form"""
    _spawn(_golden_worker, 2, str(tmp_path))
    for r in range(2):
        g = np.load(str(tmp_path / f"g{r}.npz"))
        for name in ("pairq", "soft"):
            for k in (15, 21):
                ref = pd.read_csv(os.path.join(GOLDEN, f"{name}.abd.k{k}.w1.v6.l100.csv"), header=None)
                assert (g[f"{name}{k}_names"] == ref[0].to_numpy()).all()
                assert np.array_equal(g[f"{name}{k}"], ref.drop(columns=0).to_numpy()), (name, k)


def _manifest_cases():
    import json
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return [c for c in json.load(f)["cases"] if c["tool"] == "count_kmer" and not c["holes"]]


def _every_golden_worker(rank, world, port, outdir):
    _init(rank, world, port)
    originals = {name: getattr(pdist, name) for name in ("features_sharded_mini", "count_kmers_sharded")}
    try:
        took = []

        def spy_mini(*a, **kw):
            r = originals["features_sharded_mini"](*a, **kw)
            took.append("super-k-mer" + (" masked" if r[2] is not None and r[2].masked else "") if r[2] is not None else "super-k-mer refused")
            return r

        def spy_keys(*a, **kw):
            took.append("key-partitioned")
            return originals["count_kmers_sharded"](*a, **kw)

        pdist.features_sharded_mini, pdist.count_kmers_sharded = spy_mini, spy_keys
        out = {}
        for i, case in enumerate(_manifest_cases()):
            del took[:]
            spec = case["input"]
            r1 = os.path.join(GOLDEN, spec.get("i") or spec["1"])
            r2 = os.path.join(GOLDEN, spec["2"]) if "2" in spec else None
            names, _, abd = feature.compute_features(r1, r2, case["k"], 4, case["window"], case["vsize"], case["min_len"],
                                                     device=torch.device("cuda", 0), want_tnf=False,
                                                     lowercase_is_base=case.get("jellyfish_rules", False))
            assert len(took) >= 1, case["expect"]
            out[f"names{i}"], out[f"abd{i}"], out[f"form{i}"] = np.array(names, dtype=str), abd, np.array(" + ".join(took))
        np.savez(os.path.join(outdir, f"e{rank}.npz"), **out)
    finally:
        for name, orig in originals.items():
            setattr(pdist, name, orig)
        dist.destroy_process_group()


@pytest.mark.gpu
def test_every_golden_through_compute_features_on_two_ranks(tmp_path):
    """every count_kmer case of the manifest whose table the GPU counts by itself (k = 3, 4, 5, 9, 11, 15, 21, 31), with the case's own
    input, window, vector size and minimum length, under two gloo ranks in one spawn: the matrix gathered on rank 0 (and on rank 1)
    is the reference's committed CSV, names included -- through whichever N-rank form compute_features picks (printed per case)"""
    cases = _manifest_cases()
    assert {c["k"] for c in cases} >= {3, 4, 5, 9, 11, 15, 21, 31}
    _spawn(_every_golden_worker, 2, str(tmp_path))
    ran = 0
    for r in range(2):
        g = np.load(str(tmp_path / f"e{r}.npz"))
        for i, case in enumerate(cases):
            with open(os.path.join(GOLDEN, case["expect"]), "rb") as f:
                want = f.read()
            names, abd = g[f"names{i}"].tolist(), np.ascontiguousarray(g[f"abd{i}"], dtype=np.int32)
            if r == 0:
                print(f"{case['expect']}: k={case['k']} {g[f'form{i}']}, {len(names)} rows")
            # the file the reference's tool wrote, byte for byte (its writer prints six significant digits: so does pg_write_csv_gz)
            assert abd.shape == (len(names), case["vsize"]) and len(names) == want.count(b"\n") > 0, case["expect"]
            out = str(tmp_path / "o.gz")
            _lib.check(_lib.load().pg_write_csv_gz(out.encode(), b"".join(n.encode() + b"\0" for n in names), abd.ctypes.data,
                                                   abd.shape[0], abd.shape[1]))
            with gzip.open(out, "rb") as f:
                assert f.read() == want, case["expect"]
            ran += r == 0
    assert ran == len(cases)


@pytest.mark.gpu
def test_masked_form_through_the_checked_build():
    """the masked kernels with every global store checked against its buffer (PANGAEA_LIB=checked: PG_STATUS_BOUNDS is raised on
    every rank by MiniSharded)"""
    import subprocess
    import sys
    env = dict(os.environ, PANGAEA_LIB="checked")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_dist_masked_gpu.py"),
                        "-k", "quality_masked_on_several_ranks or (soft_and_quality and not 18) or poly_a or goldens or pieces"
                              " or (at_every_k and (14 or 15 or 17 or 19))"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "no tests ran" not in r.stdout
