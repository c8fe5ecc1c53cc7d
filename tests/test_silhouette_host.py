"""The number of clusters by silhouette score, host side: the numpy restatement against scikit-learn and a hand-computed case,
the CPU (torch) form of dist_sums / silhouette_samples / silhouette_score against the restatement, choose_clusters and
cluster_barcode_reads on the CPU, and the argument checks of pg_cluster_dist_sums -- all answered before any launch."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pangaea_amd import _lib, clustering

from . import _silhouette_ref as ref


def _blobs(n_blobs=7, per=100, dim=32, seed=11):
    """Gaussian blobs of unit sigma, shuffled; every centre 30 sigma out on an axis of its own: 42 sigma between any two"""
    rs = np.random.RandomState(seed)
    centres = np.zeros((n_blobs, dim))
    centres[np.arange(n_blobs), np.arange(n_blobs)] = 30.0
    x = np.concatenate([rs.randn(per, dim) + c for c in centres]).astype(np.float32)
    truth = np.repeat(np.arange(n_blobs), per)
    perm = rs.permutation(len(x))
    return x[perm], truth[perm]


def _case(n, dim, k, empty=(), seed=0):
    """n random rows with labels in [0, k) that leave the clusters ``empty`` empty"""
    rs = np.random.RandomState(seed)
    x = rs.randn(n, dim).astype(np.float32)
    used = np.array([c for c in range(k) if c not in empty])
    labels = used[rs.randint(0, len(used), size=n)]
    labels[:len(used)] = used                                  # (every other cluster holds at least one row)
    return x, labels


# ------------------------------------------------------------------------------------------------ the restatement itself

def test_reference_equals_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rs = np.random.RandomState(3)
    x = rs.randn(300, 8)
    labels = rs.randint(0, 5, size=300)
    labels[labels == 4] = 3
    labels[0] = 4                                              # a singleton
    got = ref.silhouette_samples(x, labels, 5)
    want = metrics.silhouette_samples(x, labels)
    assert np.abs(got - want).max() <= 1e-12
    assert abs(ref.silhouette_score(x, labels, 5) - metrics.silhouette_score(x, labels)) <= 1e-12


def test_reference_on_a_hand_computed_line():
    """0 1 2 | 10 12 | 20: the mean distances by hand"""
    x = np.array([[0.], [1.], [2.], [10.], [12.], [20.]])
    labels = np.array([0, 0, 0, 1, 1, 2])
    want = np.array([(11 - 1.5) / 11, (10 - 1) / 10, (9 - 1.5) / 9, (9 - 2) / 9, (8 - 2) / 8, 0.0])
    assert np.abs(ref.silhouette_samples(x, labels, 3) - want).max() <= 1e-15
    s = ref.dist_sums(x, x, labels, 3)
    assert np.array_equal(s[0], [3., 22., 20.]) and np.array_equal(s[5], [57., 18., 0.])


# ------------------------------------------------------------------------------------------------ the CPU form

@pytest.mark.parametrize("empty", [(), (0,), (3, 4), (6,), (0, 3, 4, 6)], ids=["none", "first", "middle", "last", "all_three"])
def test_cpu_dist_sums_and_samples_with_empty_clusters(empty):
    x, labels = _case(257, 5, 7, empty=empty, seed=len(empty))
    got = clustering.dist_sums(torch.from_numpy(x), torch.from_numpy(x), torch.from_numpy(labels), 7)
    want = ref.dist_sums(x, x, labels, 7)
    assert got.dtype == torch.float64 and tuple(got.shape) == (257, 7)
    assert np.abs(got.numpy() - want).max() <= 1e-9 * want.max()
    for c in empty:
        assert (got[:, c] == 0).all()
    sil = clustering.silhouette_samples(torch.from_numpy(x), labels, 7)
    assert np.abs(sil.numpy() - ref.silhouette_samples(x, labels, 7)).max() <= 1e-9


def test_cpu_form_in_small_tiles(monkeypatch):
    """the torch form walks [query rows, reference rows] tiles: tiles far smaller than the matrix give the same sums"""
    x, labels = _case(257, 5, 7, empty=(3,), seed=4)
    t = torch.from_numpy(x)
    whole = clustering.dist_sums(t[:100], t, labels, 7)
    monkeypatch.setattr(clustering, "_TORCH_FORM_ROWS", 50)
    monkeypatch.setattr(clustering, "_TORCH_FORM_TILE", 350)
    tiled = clustering.dist_sums(t[:100], t, labels, 7)
    assert (tiled - whole).abs().max() <= 1e-12 * whole.max()
    assert np.abs(tiled.numpy() - ref.dist_sums(x[:100], x, labels, 7)).max() <= 1e-9 * float(whole.max())


def test_cpu_singleton_and_duplicate_rows():
    x, labels = _case(120, 4, 4, seed=5)
    labels[labels == 3] = 2
    labels[17] = 3                                             # the only row of cluster 3
    x[40:60] = x[40]                                           # twenty identical rows, all in one cluster
    labels[40:60] = 1
    x[5] = x[4]                                                # two identical rows in different clusters
    labels[4], labels[5] = 0, 2
    sil = clustering.silhouette_samples(torch.from_numpy(x), labels, 4).numpy()
    assert sil[17] == 0.0
    assert np.abs(sil - ref.silhouette_samples(x, labels, 4)).max() <= 1e-9
    # every row the same: a = b = 0, the quotient is not finite, the coefficient is 0
    same = np.ones((10, 3), dtype=np.float32)
    assert (clustering.silhouette_samples(torch.from_numpy(same), np.arange(10) % 2, 2) == 0).all()
    assert (ref.silhouette_samples(same, np.arange(10) % 2, 2) == 0).all()


def test_cpu_rows_restrict_the_query_side_only():
    x, labels = _case(200, 6, 5, seed=8)
    rows = np.array([3, 199, 0, 57, 58])
    full = clustering.silhouette_samples(torch.from_numpy(x), labels, 5).numpy()
    part = clustering.silhouette_samples(torch.from_numpy(x), labels, 5, rows=rows).numpy()
    assert np.array_equal(part, full[rows])                    # the reference side is still all rows
    assert np.abs(part - ref.silhouette_samples(x, labels, 5, rows=rows)).max() <= 1e-9
    assert np.abs(part - ref.silhouette_samples(x[rows], labels[rows], 5)).max() > 1e-3       # (what thinning both sides would give)


def test_refusals():
    x, labels = _case(30, 3, 3, seed=2)
    t = torch.from_numpy(x)
    with pytest.raises(ValueError, match="k = 1"):
        clustering.silhouette_samples(t, np.zeros(30, dtype=np.int64), 1)
    bad = labels.copy(); bad[7] = 3
    with pytest.raises(ValueError, match="outside"):
        clustering.silhouette_samples(t, bad, 3)
    bad[7] = -1
    with pytest.raises(ValueError, match="outside"):
        clustering.silhouette_score(t, bad, 3)
    with pytest.raises(ValueError, match="fewer than two"):
        clustering.silhouette_samples(t, np.full(30, 2), 3)
    with pytest.raises(ValueError, match="labels for"):
        clustering.silhouette_samples(t, labels[:-1], 3)


def test_sampled_score_leaves_the_global_generator_alone_and_depends_on_the_seed_only():
    x, labels = _case(400, 4, 6, seed=9)
    t = torch.from_numpy(x)
    np.random.seed(77)
    before = np.random.get_state()
    a = clustering.silhouette_score(t, labels, 6, sample=50, seed=4)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    np.random.seed(123)                                        # another global state: the same sample
    assert clustering.silhouette_score(t, labels, 6, sample=50, seed=4) == a
    assert clustering.silhouette_score(t, labels, 6, sample=50, seed=5) != a
    rows = np.sort(np.random.RandomState(4).choice(400, 50, replace=False))
    assert abs(a - ref.silhouette_score(x, labels, 6, rows=rows)) <= 1e-9
    assert abs(clustering.silhouette_score(t, labels, 6, sample=400) - ref.silhouette_score(x, labels, 6)) <= 1e-9


# ------------------------------------------------------------------------------------------------ the sweep

def test_choose_clusters_finds_seven_blobs():
    x, truth = _blobs()
    np.random.seed(2021)
    before = np.random.get_state()
    k, table = clustering.choose_clusters(x, range_step=(4, 20, 3), device="cpu")
    after = np.random.get_state()
    assert k == 7
    assert [row[0] for row in table] == [4, 7, 10, 13, 16, 19]
    best = dict((row[0], row[1]) for row in table)
    assert best[7] == max(best.values()) and best[7] > 0.8
    assert all(len(row) == 4 and row[3] == row[0] for row in table)
    assert np.array_equal(before[1], after[1]) and before[2] == after[2]           # the fits' draws are put back


def test_choose_clusters_stops_after_patience():
    x, _ = _blobs()
    np.random.seed(5)
    k, table = clustering.choose_clusters(x, range_step=(4, 100, 3), patience=2, device="cpu")
    assert k == 7
    assert [row[0] for row in table] == [4, 7, 10, 13]         # two entries after the best one


def test_choose_clusters_never_exceeds_n_minus_one():
    rs = np.random.RandomState(0)
    x = rs.randn(9, 4).astype(np.float32)
    np.random.seed(1)
    k, table = clustering.choose_clusters(x, range_step=(4, 100, 3), patience=50, device="cpu")
    assert [row[0] for row in table] == [4, 7] and k in (4, 7)
    with pytest.raises(ValueError, match="at least 6"):
        clustering.choose_clusters(x[:5], device="cpu")


def test_choose_clusters_ends_where_the_reducer_leaves_too_few_points():
    """2 500 rows in five tight groups collapse onto five reduced points: k = 8 cannot be fitted, the sweep ends with what it has"""
    rs = np.random.RandomState(4)
    centres = np.zeros((5, 32))
    centres[np.arange(5), np.arange(5)] = 30.0
    x = np.concatenate([rs.randn(500, 32) * 1e-3 + c for c in centres]).astype(np.float32)
    np.random.seed(3)
    k, table = clustering.choose_clusters(x, range_step=(2, 100, 3), device="cpu")
    assert k == 5 and [row[0] for row in table] == [2, 5]
    with pytest.raises(clustering.TooFewReducedPoints):        # nothing fitted at all: the error is the caller's
        clustering.choose_clusters(x, range_step=(8, 100, 3), device="cpu")


# ------------------------------------------------------------------------------------------------ step 3

def _barcode(i):
    return "".join("ACGT"[(i >> (2 * j)) & 3] for j in range(6))


def _prepare_step3(tmp_path, n_blobs=7, per=10):
    x, _ = _blobs(n_blobs=n_blobs, per=per)
    model, clus = tmp_path / "2.vae", tmp_path / "3.clustering"
    model.mkdir(); clus.mkdir()
    barcodes = np.array([_barcode(i) for i in range(len(x))])
    np.savez(model / "latent.npz", x)
    np.savez(model / "barcodes.npz", barcodes)
    fq = tmp_path / "reads.fq"
    fq.write_text("".join(f"@r{i} BX:Z:{b}-1\nACGTACGT\n+\nIIIIIIII\n@r{i} BX:Z:{b}-1\nTTGCAAGG\n+\nIIIIIIII\n" for i, b in enumerate(barcodes)))
    return model, clus, str(fq), barcodes


def test_cluster_barcode_reads_by_silhouette(tmp_path):
    model, clus, fq, barcodes = _prepare_step3(tmp_path)
    args = argparse.Namespace(clusters=None, auto_clusters="silhouette", cluster_range="4,20,3", reads1="", reads2="", interleaved_reads=fq,
                              metaphlan_db="")
    np.random.seed(2021)
    clustering.cluster_barcode_reads(args, str(model), str(clus), str(tmp_path / "no_such_checkout"), device="cpu")
    lines = (clus / "silhouette.tsv").read_text().splitlines()
    assert lines[0] == "k\tscore\tinertia\tclusters"
    rows = [line.split("\t") for line in lines[1:]]
    assert [int(r[0]) for r in rows] == [4, 7, 10, 13, 16, 19]
    assert all(len(r[1].split(".")[1]) == 6 for r in rows)
    assert max(rows, key=lambda r: float(r[1]))[0] == "7"
    labels = np.load(clus / "clusters.npz")["arr_0"]
    assert len(labels) == len(barcodes) and len(np.unique(labels)) == 7
    assert len((clus / "clusters.tsv").read_text().splitlines()) == 7
    assert (clus / "clustering_finished").is_file()
    for lab in np.unique(labels):
        assert (clus / f"cluster_bin{lab}.fq").is_file()
    # the chosen K gives what -c K gives: the sweep leaves the generator where it found it
    clus2 = tmp_path / "again"
    clus2.mkdir()
    np.random.seed(2021)
    clustering.cluster_barcode_reads(argparse.Namespace(**dict(vars(args), clusters=7)), str(model), str(clus2), str(tmp_path), device="cpu")
    assert np.array_equal(np.load(clus2 / "clusters.npz")["arr_0"], labels)
    assert not (clus2 / "silhouette.tsv").exists()


def test_cluster_barcode_reads_without_the_flag_still_asks_for_the_script(tmp_path):
    model, clus, fq, _ = _prepare_step3(tmp_path)
    for extra in ({}, {"auto_clusters": "metaphlan"}):
        args = argparse.Namespace(clusters=None, reads1="", reads2="", interleaved_reads=fq, metaphlan_db="", **extra)
        with pytest.raises(FileNotFoundError, match=r"number of clusters \(-c\) not given and scripts/calculate_diversity.sh not found"):
            clustering.cluster_barcode_reads(args, str(model), str(clus), str(tmp_path / "no_such_checkout"))
    assert not (clus / "silhouette.tsv").exists()


def test_pangaea_flags():
    from pangaea_amd.pangaea import build_parser
    p = build_parser()
    a = p.parse_args(["-o", "out"])
    assert a.auto_clusters == "metaphlan" and a.cluster_range == "4,100,3"
    a = p.parse_args(["-o", "out", "--auto_clusters", "silhouette", "--cluster_range", "4,20,3"])
    assert a.auto_clusters == "silhouette" and a.cluster_range == "4,20,3"
    with pytest.raises(SystemExit):
        p.parse_args(["-o", "out", "--auto_clusters", "elbow"])


# ------------------------------------------------------------------------------------------------ the C entry, no device

def _call(L, q=1, n_q=4, x=1, n_x=4, dim=32, seg=1, k=2, n_splits=0, out=1, work=None, work_bytes=0):
    """pg_cluster_dist_sums with host buffers standing in for device pointers: every case here is answered before they are used"""
    buf = (C.c_double * 4096)()
    p = C.addressof(buf)
    return L.pg_cluster_dist_sums(p if q else None, n_q, p if x else None, n_x, dim, p if seg else None, k, n_splits, p if out else None,
                                  p if work else None, work_bytes, None)


@pytest.mark.parametrize("kw,name", [
    (dict(n_q=-1), "n_q"), (dict(n_x=-1), "n_x"), (dict(dim=0), "dim"), (dict(dim=257), "dim"), (dict(k=0), "k"), (dict(k=4097), "k"),
    (dict(n_splits=-1), "n_splits"), (dict(n_splits=65), "n_splits"), (dict(q=0), "q is null"), (dict(x=0), "x is null"),
    (dict(seg=0), "seg is null"), (dict(out=0), "out is null"), (dict(n_splits=3), "workspace is null"),
    (dict(n_splits=3, work=1, work_bytes=3 * 4 * 2 * 8 - 1), "workspace_bytes"), (dict(work_bytes=-1), "workspace_bytes")])
def test_c_entry_refuses_bad_arguments_by_name(kw, name):
    L = _lib.load()
    assert _call(L, **kw) == -1                                # PG_EINVAL
    msg = L.pg_last_error().decode()
    assert "pg_cluster_dist_sums" in msg and name in msg, msg


def test_c_entry_no_rows_is_a_no_op_and_the_abi_stays():
    L = _lib.load()
    assert L.pg_abi_version() == _lib.ABI_VERSION == 9
    assert L.pg_cluster_dist_sums(None, 0, None, 5, 32, None, 2, 0, None, None, 0, None) == 0
    assert L.pg_cluster_dist_sums(None, 5, None, 0, 32, None, 2, 0, None, None, 0, None) == 0
    assert L.pg_cluster_dist_sums(None, 0, None, 0, 7, None, 4096, 64, None, None, 0, None) == 0
    ws = L.pg_cluster_dist_sums_workspace_bytes
    assert ws(0, 100, 5, 3) == 0 and ws(100, 0, 5, 3) == 0
    assert ws(10, 100, 5, 1) == 0 and ws(10, 100, 5, 3) == 3 * 10 * 5 * 8 and ws(65, 1031, 7, 64) == 64 * 65 * 7 * 8
    # the library's own choice: one split when the query rows alone fill the device, never more than 64 otherwise
    assert ws(1_000_000, 1_000_000, 40, 0) == 0
    chosen = ws(16384, 1_000_000, 40, 0) // (16384 * 40 * 8)
    assert 2 <= chosen <= 64 and ws(16384, 1_000_000, 40, 0) == chosen * 16384 * 40 * 8
    assert 0 <= ws(1, 1, 1, 0) <= 64 * 8
    for bad in ((-1, 1, 2, 0), (1, -1, 2, 0), (1, 1, 0, 0), (1, 1, 4097, 0), (1, 1, 2, 65)):
        assert ws(*bad) == -1 and "pg_cluster_dist_sums_workspace_bytes" in L.pg_last_error().decode()
