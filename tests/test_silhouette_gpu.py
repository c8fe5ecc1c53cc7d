"""pg_cluster_dist_sums (csrc/cluster.hip) and the silhouette on top of it, on the GPU, against the numpy float64 restatement
(tests/_silhouette_ref.py) on the same float32 values.

The tolerance is derived, not tuned.  Per sum, relative (dim + 16) * 2^-24: the differences (1 ulp), the squares, a dim-term
float32 accumulation of positives (<= dim ulp), halved by the square root, which adds its own ulp, and the float32 partial sums of
at most PG_CLUSTER_GROUP = 8 distances; exactly 0 where the reference is 0.  Per s_i, absolute 4 * (dim + 16) * 2^-24: twice the
relative bound of a plus that of b, with a factor 2 of room."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pangaea_amd import _lib, clustering

from . import _silhouette_ref as ref
from .conftest import ROOT
from .test_silhouette_host import _barcode, _blobs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GROUP = _lib.CLUSTER_GROUP        # PG_CLUSTER_GROUP: the reference rows of one float32 partial sum -- the only tile of the kernel
GUARD = 5                         # doubles in front of and behind the output that the kernel must leave alone
SENTINEL = -12345.0


def _bound(dim):
    return (dim + 16) * 2.0 ** -24


def _raw(q, x, labels, k, n_splits=0):
    """the C entry on its own: x sorted by label here (numpy), the output between guard words, which are checked"""
    L = _lib.load()
    order = np.argsort(labels, kind="stable")
    seg = np.zeros(k + 1, dtype=np.int64)
    seg[1:] = np.cumsum(np.bincount(labels, minlength=k))
    n_q, n_x, dim = len(q), len(x), q.shape[1]
    dq = torch.from_numpy(np.ascontiguousarray(q)).to(DEV)
    dx = torch.from_numpy(np.ascontiguousarray(x[order])).to(DEV)
    dseg = torch.from_numpy(seg).to(DEV)
    buf = torch.full((n_q * k + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    out = buf[GUARD:GUARD + n_q * k]
    need = _lib.check(L.pg_cluster_dist_sums_workspace_bytes(n_q, n_x, k, n_splits))
    assert need <= max(n_splits, _lib.CLUSTER_MAX_SPLITS) * n_q * k * 8
    work = torch.full((need // 8 + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    _lib.check(L.pg_cluster_dist_sums(dq.data_ptr(), n_q, dx.data_ptr(), n_x, dim, dseg.data_ptr(), k, n_splits, out.data_ptr(),
                                      work[GUARD:].data_ptr() if need else None, need, None))
    torch.cuda.synchronize()
    host, wh = buf.cpu().numpy(), work.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n_q * k:] == SENTINEL).all(), "a store outside the output"
    assert (wh[:GUARD] == SENTINEL).all() and (wh[GUARD + need // 8:] == SENTINEL).all(), "a store outside the workspace"
    return host[GUARD:GUARD + n_q * k].reshape(n_q, k)


def _check(got, want, dim, what):
    zero = want == 0
    assert (got[zero] == 0).all(), f"{what}: a sum that must be exactly 0 is not"
    rel = np.abs(got[~zero] - want[~zero]) / want[~zero]
    worst = float(rel.max()) if rel.size else 0.0
    print(f"dist_sums {what}: worst relative error {worst * 2 ** 24:.2f} x 2^-24 (bound {dim + 16})")
    assert worst <= _bound(dim), (what, worst)


def _random(n_q, n_x, dim, k, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    q = (rs.randn(n_q, dim) * scale).astype(np.float32)
    x = (rs.randn(n_x, dim) * scale).astype(np.float32)
    return q, x, rs.randint(0, k, size=n_x)


def _by_sizes(sizes, dim, n_q, seed):
    """reference rows in clusters of the given sizes (shuffled), queries of their own"""
    rs = np.random.RandomState(seed)
    labels = rs.permutation(np.repeat(np.arange(len(sizes)), sizes))
    return rs.randn(n_q, dim).astype(np.float32), rs.randn(len(labels), dim).astype(np.float32), labels


# n_q around a wavefront (64) and a workgroup (256); n_x from a single row to several hundred groups
@pytest.mark.parametrize("n_q,n_x", [(1, 1), (1, 300), (63, 64), (65, 257), (300, 1), (513, 1031)], ids=lambda v: str(v))
@pytest.mark.parametrize("dim", [1, 3, 31, 32, 33, 64, 256])
def test_kernel_against_float64(dim, n_q, n_x):
    q, x, labels = _random(n_q, n_x, dim, 3, seed=dim * 7 + n_q + n_x)
    _check(_raw(q, x, labels, 3), ref.dist_sums(q, x, labels, 3), dim, f"dim {dim} ({n_q}, {n_x})")


@pytest.mark.parametrize("n_x", [GROUP - 1, GROUP, GROUP + 1, 2 * GROUP, 2 * GROUP + 1])
@pytest.mark.parametrize("dim", [5, 32])
def test_kernel_either_side_of_a_group(dim, n_x):
    """PG_CLUSTER_GROUP reference rows make one float32 partial sum: one cluster of a group less one, a group, a group and one"""
    q, x, _ = _random(65, n_x, dim, 1, seed=n_x)
    _check(_raw(q, x, np.zeros(n_x, dtype=np.int64), 1), ref.dist_sums(q, x, np.zeros(n_x, dtype=np.int64), 1), dim, f"dim {dim} n_x {n_x}")


@pytest.mark.parametrize("k", [1, 2, 7, 100])
@pytest.mark.parametrize("dim", [32, 33])
def test_kernel_cluster_counts(dim, k):
    q, x, labels = _random(65, 257, dim, k, seed=k)
    _check(_raw(q, x, labels, k), ref.dist_sums(q, x, labels, k), dim, f"dim {dim} k {k}")


@pytest.mark.parametrize("dim", [32, 20])
def test_kernel_most_clusters_singletons_or_empty(dim):
    q, x, labels = _random(70, 5000, dim, 4096, seed=4096)
    sizes = np.bincount(labels, minlength=4096)
    assert (sizes == 0).sum() > 500 and (sizes == 1).sum() > 500
    _check(_raw(q, x, labels, 4096), ref.dist_sums(q, x, labels, 4096), dim, f"dim {dim} k 4096")


@pytest.mark.parametrize("dim", [32, 33])
def test_kernel_cluster_structure(dim):
    """empty clusters at both ends and two in a row in the middle; clusters that end on a group boundary (8, 16) and that do not
    (5, 3); one that spans several groups (43)"""
    sizes = [0, GROUP, 0, 0, 2 * GROUP, 5, 5 * GROUP + 3, 3, 0]
    q, x, labels = _by_sizes(sizes, dim, 65, seed=dim)
    got = _raw(q, x, labels, len(sizes))
    _check(got, ref.dist_sums(q, x, labels, len(sizes)), dim, f"dim {dim} structure")
    assert (got[:, [0, 2, 3, 8]] == 0).all()


SPLIT_SIZES = [343, 100, 300, 0, 88, 150, 50]          # of 1 031 rows in 3 splits (cuts at 343 and 687): the first cut ON a cluster
                                                        # boundary, the second INSIDE the third cluster


@pytest.mark.parametrize("dim", [32, 7])
def test_kernel_splits(dim):
    assert sum(SPLIT_SIZES) == 1031 and 1031 * 1 // 3 == 343 and 443 < 1031 * 2 // 3 < 743
    q, x, labels = _by_sizes(SPLIT_SIZES, dim, 65, seed=3)
    want = ref.dist_sums(q, x, labels, 7)
    for n_splits in (0, 1, 3, 64):
        got = _raw(q, x, labels, 7, n_splits)
        _check(got, want, dim, f"dim {dim} n_splits {n_splits}")
        assert np.array_equal(got, _raw(q, x, labels, 7, n_splits)), f"n_splits {n_splits}: two runs differ"
    # more splits than reference rows: most pieces are empty
    q, x, labels = _random(5, 3, dim, 2, seed=1)
    _check(_raw(q, x, labels, 2, 64), ref.dist_sums(q, x, labels, 2), dim, f"dim {dim} 64 splits of 3 rows")


@pytest.mark.parametrize("dim", [32, 6])
def test_kernel_duplicates_and_own_rows(dim):
    """queries that ARE reference rows, and a cluster made of copies of one query: its sum is exactly 0"""
    _, x, labels = _random(1, 300, dim, 4, seed=12)
    labels[labels == 3] = 2
    x[100:120] = x[100]
    labels[100:120] = 3                                        # cluster 3: twenty copies of row 100
    x[7] = x[8]
    q = x[[100, 7, 8, 0, 299]].copy()
    got = _raw(q, x, labels, 4)
    _check(got, ref.dist_sums(q, x, labels, 4), dim, f"dim {dim} duplicates")
    assert got[0, 3] == 0.0 and got[1, 3] > 0.0
    assert np.array_equal(got[1], got[2])


@pytest.mark.parametrize("scale", [1e-3, 1e3])
@pytest.mark.parametrize("dim", [32, 256])
def test_kernel_small_and_large_values(dim, scale):
    q, x, labels = _random(65, 257, dim, 3, seed=5, scale=scale)
    got = _raw(q, x, labels, 3)
    assert np.isfinite(got).all() and (got > 0).all()
    _check(got, ref.dist_sums(q, x, labels, 3), dim, f"dim {dim} scale {scale}")


def test_python_layer_copies_what_is_not_contiguous_float32():
    """a non-contiguous slice (every other row, the left half of the columns) and float64 input are COPIED to contiguous
    float32, not refused: the same sums as for the contiguous rows"""
    rs = np.random.RandomState(2)
    wide = torch.from_numpy(rs.randn(600, 64).astype(np.float32)).to(DEV)
    labels = torch.from_numpy(rs.randint(0, 5, size=300)).to(DEV)
    x, q = wide[::2, :32], wide[1::4, :32]
    assert not x.is_contiguous() and not q.is_contiguous()
    got = clustering.dist_sums(q, x, labels, 5)
    assert torch.equal(got, clustering.dist_sums(q.contiguous(), x.contiguous(), labels, 5))
    assert torch.equal(got, clustering.dist_sums(q.double(), x.double(), labels, 5))
    _check(got.cpu().numpy(), ref.dist_sums(q.cpu().numpy(), x.cpu().numpy(), labels.cpu().numpy(), 5), 32, "python layer, slices")
    with pytest.raises(ValueError, match="labels outside"):    # seg is built here: its shape is this layer's to check
        clustering.dist_sums(q, x, labels + 1, 5)
    assert tuple(clustering.dist_sums(q[:0], x, labels, 5).shape) == (0, 5)
    assert (clustering.dist_sums(q, x[:0], labels[:0], 5) == 0).all()


@pytest.fixture(scope="module")
def fitted():
    """1 500 rows in 9 blobs that overlap, labelled by their blob (one of them a single row) -- and the reference's coefficients,
    computed once"""
    rs = np.random.RandomState(21)
    centres = rs.randn(9, 32) * 1.5
    x = np.concatenate([rs.randn(n, 32) + c for n, c in zip([400, 300, 250, 200, 150, 100, 60, 39, 1], centres)]).astype(np.float32)
    labels = np.concatenate([np.full(n, c) for c, n in enumerate([400, 300, 250, 200, 150, 100, 60, 39, 1])])
    perm = rs.permutation(len(x))
    x, labels = x[perm], labels[perm]
    return x, labels, ref.silhouette_samples(x, labels, 9)


def test_python_layer_samples_and_score(fitted):
    x, labels, want = fitted
    t = torch.from_numpy(x).to(DEV)
    got = clustering.silhouette_samples(t, labels, 9)
    assert got.dtype == torch.float64 and got.is_cuda
    err = float(np.abs(got.cpu().numpy() - want).max())
    print(f"silhouette_samples N 1500 k 9: worst |s_i - reference| = {err * 2 ** 24:.2f} x 2^-24 (bound {4 * 48})")
    assert err <= 4 * _bound(32)
    assert abs(clustering.silhouette_score(t, labels, 9) - want.mean()) <= 4 * _bound(32)
    state = np.random.get_state()
    sampled = clustering.silhouette_score(t, labels, 9, sample=400, seed=3)
    assert np.array_equal(state[1], np.random.get_state()[1])
    rows = np.sort(np.random.RandomState(3).choice(1500, 400, replace=False))
    assert abs(sampled - want[rows].mean()) <= 4 * _bound(32)


def test_torch_form_in_a_child_process_agrees(fitted, tmp_path):
    """PG_SILHOUETTE_KERNEL=0, the A/B partner: the same sums from torch.cdist in float64, in a process of its own"""
    x, labels, _ = fitted
    np.save(tmp_path / "x.npy", x)
    np.save(tmp_path / "labels.npy", labels)
    code = ("import sys, numpy as np, torch\n"
            "from pangaea_amd import _lib, clustering\n"
            "d = sys.argv[1]\n"
            "L = _lib.load()\n"
            "def boom(*a): raise AssertionError('the kernel ran')\n"
            "L.pg_cluster_dist_sums = boom\n"
            "x = torch.from_numpy(np.load(d + '/x.npy')).cuda()\n"
            "s = clustering.dist_sums(x[:500], x, np.load(d + '/labels.npy'), 9)\n"
            "assert s.is_cuda\n"
            "np.save(d + '/sums.npy', s.cpu().numpy())\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], cwd=ROOT, env=dict(os.environ, PG_SILHOUETTE_KERNEL="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    torch_form = np.load(tmp_path / "sums.npy")
    t = torch.from_numpy(x).to(DEV)
    kernel = clustering.dist_sums(t[:500], t, labels, 9).cpu().numpy()
    _check(kernel, torch_form, 32, "kernel against the torch form")
    assert np.abs(torch_form - ref.dist_sums(x[:500], x, labels, 9)).max() <= 1e-9 * torch_form.max()


def test_choose_clusters_on_the_gpu():
    x, _ = _blobs()
    np.random.seed(2021)
    k, table = clustering.choose_clusters(x, range_step=(4, 20, 3))
    assert k == 7 and [row[0] for row in table] == [4, 7, 10, 13, 16, 19]
    k, table = clustering.choose_clusters(torch.from_numpy(x).to(DEV), range_step=(4, 100, 3), patience=2, sample=300, seed=1)
    assert k == 7 and [row[0] for row in table] == [4, 7, 10, 13]


def test_step_3_end_to_end_without_c(tmp_path):
    """pangaea.py -st 3 --auto_clusters silhouette on a prepared 2.vae/: 700 barcodes in 7 blobs, a small FASTQ"""
    from pangaea_amd import pangaea
    x, _ = _blobs()
    out = tmp_path / "out"
    (out / "2.vae").mkdir(parents=True)
    barcodes = np.array([_barcode(i) for i in range(len(x))])
    np.savez(out / "2.vae" / "latent.npz", x)
    np.savez(out / "2.vae" / "barcodes.npz", barcodes)
    fq = tmp_path / "reads.fq"
    fq.write_text("".join(f"@r{i} BX:Z:{b}-1\nACGTACGT\n+\nIIIIIIII\n@r{i} BX:Z:{b}-1\nTTGCAAGG\n+\nIIIIIIII\n" for i, b in enumerate(barcodes)))
    pangaea.main(["-i", str(fq), "-o", str(out), "-st", "3", "--auto_clusters", "silhouette", "--cluster_range", "4,20,3",
                  "--reference_src", str(tmp_path / "no_such_checkout")])
    clus = out / "3.clustering"
    lines = (clus / "silhouette.tsv").read_text().splitlines()
    assert lines[0] == "k\tscore\tinertia\tclusters" and [line.split("\t")[0] for line in lines[1:]] == ["4", "7", "10", "13", "16", "19"]
    labels = [line.split("\t")[0] for line in (clus / "clusters.tsv").read_text().splitlines()]
    assert len(labels) == 7 and (clus / "clustering_finished").is_file()
    for lab in labels:
        assert (clus / f"cluster_bin{lab}.fq").stat().st_size > 0
    assert len([f for f in os.listdir(clus) if f.endswith(".fq")]) == 7
