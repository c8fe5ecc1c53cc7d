"""Clustering layer -- counterpart of /root/reference/src/clustering.py:14-129 with RPH-KMeans on the GPU.

``clustering_rph_kmeans(embedding, k)`` keeps the reference's call (``RPHKMeans(n_init=20, n_clusters=k)``,
clustering.py:14-19).  The algorithm is the vendored library's (third_parties/rph_kmeans):
  * bucket width w = half the median of 1 000 random paired distances        (point_reducer_base.py:35-48)
  * repeat until <= 2 000 points: 5 random projections N(0, 1/w) + U(0,1) offsets, truncate to int32, merge
    the points that share all 5 integers into their weighted mean            (point_reducer_cy.py:47-76,
                                                                               _point_reducer_cy_lib.cpp:5-28, .h:52-68)
  * weighted k-means on the skeleton -> initial centres                        (rph_kmeans_.py:116-129)
  * Lloyd iterations on ALL points from those centres, best inertia of n_init (rph_kmeans_.py:143-162)
Where it runs: everything on the device -- projections, bucketing (``torch.unique`` over the 5-integer rows), weighted
merges, the weighted skeleton k-means (greedy k-means++ seeding with sklearn's 2 + ln k local trials, then weighted
Lloyd) and the Lloyd distance / assignment / update steps over all points (the [N,32]x[k,32] distance step is a GEMM +
row argmin on rows and centres with the column mean taken off, as sklearn's fit does: in float32 the GEMM form of the distance
cancels on rows that sit away from the origin, see ``_sq_dists``).  Nothing but the final labels returns to the host (and the
2 x 1 000 rows behind the bucket width, so that w is numpy's float64 value on every device).  Random draws come from numpy's
global generator in the reference's order (``init_all`` seeds it; the device generator of the k-means++ seeding is seeded from it), but bucket numbering follows
``torch.unique`` instead of ``unordered_map`` iteration, so labels are NOT bit-comparable with the reference
 -- parity is by inertia and adjusted Rand index.

Without ``-c``: ``choose_clusters`` picks k by a silhouette sweep (``--auto_clusters silhouette``), its O(N^2) distance sums in
one HIP kernel (``dist_sums``: pg_cluster_dist_sums); the sweep's own draws are put back, so the fit that follows is ``-c K``'s.
"""
from __future__ import annotations

import logging
import math
import os
import warnings
from collections import defaultdict

import numpy as np
import torch

from .utils import run_cmd


def _sq_dists(x: torch.Tensor, c: torch.Tensor, x2: torch.Tensor | None = None) -> torch.Tensor:
    """squared euclidean distances [N, K] in the dtype of x (the distance step): |x|^2 - 2 x.c + |c|^2, a GEMM.  In float32 the
    three terms are each as large as |x|^2 and |c|^2, so the result is off by ~ (dim + 3) 2^-24 (|x| + |c|)^2 whatever the
    distance is: callers pass rows and centres with the column mean of the rows taken off (``_centred``), as scikit-learn does,
    so that this size is the spread of the data and not its distance from the origin"""
    if x2 is None:
        x2 = (x * x).sum(1, keepdim=True)
    d = x2 - 2.0 * (x @ c.t()) + (c * c).sum(1)[None, :]
    return d.clamp_(min=0)


def _centred(x: torch.Tensor, mean: torch.Tensor | None = None):
    """(x - m, m): the rows with their column mean (or the ``mean`` given, float64) taken off, m rounded to the dtype of x.  Any
    vector near the mean serves as long as the SAME one is added back: the rounding of m costs nothing"""
    if mean is None:
        mean = x.mean(0, dtype=torch.float64) if x.shape[0] else torch.zeros(x.shape[1], dtype=torch.float64, device=x.device)
    m = mean.to(x.dtype)
    return x - m, m


def _uncentred(c: torch.Tensor, m: torch.Tensor):
    """(centres in the caller's coordinates, the same centres with m taken off again): the second is what the LAST distance
    step uses, so that labels and inertia belong to the centres that are handed back and not to centres 2^-24 |m| beside them"""
    out = (c.double() + m.double()).to(c.dtype)
    return out, (out.double() - m.double()).to(c.dtype)


def _all_reduce(t: torch.Tensor, group, op=None) -> torch.Tensor:
    """in-place all-reduce of a small tensor over the ranks that share the rows (gloo cannot take device tensors: staged)"""
    import torch.distributed as dist
    op = dist.ReduceOp.SUM if op is None else op
    if t.is_cuda and dist.get_backend(group) == "gloo":
        h = t.cpu()
        dist.all_reduce(h, op=op, group=group)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=op, group=group)
    return t


@torch.no_grad()
def lloyd(x: torch.Tensor, centers: torch.Tensor, max_iter: int = 300, tol: float = 1e-4, sample_weight: torch.Tensor | None = None,
          group=None, sharded: bool = False):
    """sklearn ``KMeans(init=centers, n_init=1)`` semantics (algorithm "lloyd"): the column mean of x is taken off the rows and
    the centres before the first step and added back to the centres at the end (the float32 distance step cancels otherwise:
    ``_sq_dists``); stop when the labels repeat or the squared centre shift falls below tol * mean feature variance; an empty
    cluster takes the point farthest from its centre (the points in descending order of that distance, stable).  The inertia is
    summed over the rows in float64.  Returns (labels int64 [N], centers [K,D] in the coordinates of x, inertia float, n_iter).

    ``sharded`` (rph_kmeans_.py:152-160 runs this on one matrix): ``x`` holds THIS rank's rows only.  Distances and
    assignments are local; per iteration one all-reduce sums the [K, D] coordinate sums and the [K] counts of all ranks
    (K x (D + 1) values: 5 KB for K = 40, D = 32), a second, one-word one agrees on "no label changed anywhere"; the feature
    variance behind the tolerance, the candidates for an empty cluster and the final inertia are reduced the same way; the mean
    that is taken off is the all-reduced one, the same vector on every rank.
    Every rank ends with the same centres, inertia and iteration count, and with the labels of its own rows."""
    n, dim = x.shape
    k = centers.shape[0]
    w = torch.ones(n, dtype=x.dtype, device=x.device) if sample_weight is None else sample_weight.to(x)
    if sharded:
        import torch.distributed as dist
        mom = torch.cat([x.double().sum(0), (x.double() ** 2).sum(0), torch.tensor([float(n)], dtype=torch.float64, device=x.device)])
        _all_reduce(mom, group)
        n_all = float(mom[-1].item())
        mean = mom[:dim] / n_all
        tol_abs = float((mom[dim:2 * dim] / n_all - mean * mean).clamp(min=0).mean().item()) * tol
        x, m = _centred(x, mean)
    else:
        x, m = _centred(x)
        tol_abs = float(x.var(dim=0, unbiased=False).mean().item()) * tol if n else 0.0
    x2 = (x * x).sum(1, keepdim=True)
    centers = (centers.to(device=x.device, dtype=torch.float64) - m.double()).to(x.dtype)
    light = (w == 0) if sample_weight is not None and not sharded else None
    if light is not None and not bool(light.any()):
        light = None
    labels_old = None
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        d = _sq_dists(x, centers, x2)
        mind, labels = (d.min(dim=1) if n else (x.new_zeros(0), torch.zeros(0, dtype=torch.int64, device=x.device)))
        sums = torch.zeros((k, dim), dtype=x.dtype, device=x.device).index_add_(0, labels, x * w[:, None])
        cnt = torch.zeros(k, dtype=x.dtype, device=x.device).index_add_(0, labels, w)
        if sharded:
            both = torch.cat([sums, cnt[:, None]], dim=1)
            _all_reduce(both, group)
            sums, cnt = both[:, :dim].contiguous(), both[:, dim].contiguous()
        empty = torch.nonzero(cnt == 0).flatten()
        if empty.numel() and not sharded:                   # relocate empty clusters to the farthest points
            far = torch.argsort(mind, descending=True, stable=True)[:empty.numel()]
            for e, f in zip(empty.tolist(), far.tolist()):
                old = int(labels[f])
                sums[old] -= x[f] * w[f]; cnt[old] -= w[f]
                sums[e] = x[f] * w[f]; cnt[e] = w[f]
                labels[f] = e
        elif empty.numel():
            # the same, over all ranks' rows: every rank offers its own farthest points (distance, weight, label, owner, index,
            # coordinates), the offers are gathered and every rank applies the same relocations to the reduced sums; the owner
            # of a relocated point also changes that point's label
            n_e = int(empty.numel())
            me, world = dist.get_rank(group), dist.get_world_size(group)
            offer = torch.full((n_e, 5 + dim), -1.0, dtype=torch.float64, device=x.device)
            take = min(n_e, n)
            if take:
                far = torch.argsort(mind, descending=True, stable=True)[:take]
                offer[:take, 0] = mind[far].double(); offer[:take, 1] = w[far].double(); offer[:take, 2] = labels[far].double()
                offer[:take, 3] = float(me); offer[:take, 4] = far.double(); offer[:take, 5:] = x[far].double()
            offers = torch.zeros((world, n_e, 5 + dim), dtype=torch.float64, device=x.device)
            offers[me] = offer
            _all_reduce(offers, group)                      # (a sum over one-hot rank slots = an all-gather, staged like the rest)
            flat = offers.view(-1, 5 + dim)
            order = torch.argsort(flat[:, 0], descending=True, stable=True)[:n_e]
            for e, row in zip(empty.tolist(), flat[order].tolist()):
                if row[0] < 0:
                    continue                                # (fewer points than empty clusters)
                old, wf = int(row[2]), row[1]
                xf = torch.tensor(row[5:], dtype=x.dtype, device=x.device)
                sums[old] -= xf * wf; cnt[old] -= wf
                sums[e] = xf * wf; cnt[e] = wf
                if int(row[3]) == me:
                    labels[int(row[4])] = e
        new_centers = sums / cnt.clamp(min=1e-30)[:, None]
        if light is not None and labels_old is not None and bool(((labels == labels_old) | light).all()):
            # only rows of weight 0 changed their cluster: the sums are those of the step before, and the centres are taken from
            # it -- atomics that add in another order would make a shift of exactly 0 into one of a few ulps, and one more step
            new_centers = centers
        shift = float(((new_centers - centers) ** 2).sum().item())
        centers = new_centers
        same = labels_old is not None and torch.equal(labels, labels_old)
        if sharded:
            flag = torch.tensor([1 if same else 0], dtype=torch.int32, device=x.device)
            same = bool(_all_reduce(flag, group, dist.ReduceOp.MIN).item())
        if same:
            break
        labels_old = labels
        if shift <= tol_abs:
            break
    out, centers = _uncentred(centers, m)
    d = _sq_dists(x, centers, x2)
    mind, labels = (d.min(dim=1) if n else (x.new_zeros(0), torch.zeros(0, dtype=torch.int64, device=x.device)))
    total = (mind.double() * w.double()).sum().reshape(1)
    if sharded:
        _all_reduce(total, group)
    return labels, out, float(total.item()), n_iter


@torch.no_grad()
def kmeans_plusplus(x: torch.Tensor, w: torch.Tensor, k: int, gen: torch.Generator) -> torch.Tensor:
    """greedy k-means++ seeding with sample weights, as sklearn's ``_kmeans_plusplus`` (the seeding inside the reference's
    ``KMeans(n_clusters=k).fit_predict(reduced_X, sample_weight)``, rph_kmeans_.py:121-124): the first centre is drawn in
    proportion to the weights, every further one is the best of 2 + ln k candidates drawn in proportion to weight x squared
    distance to the nearest centre so far (distances between centred rows: ``_sq_dists``).  Returns centres [k, D], rows of x."""
    n_trials = 2 + int(math.log(k))
    centers = torch.empty((k, x.shape[1]), dtype=x.dtype, device=x.device)
    first = torch.multinomial(w / w.sum(), 1, generator=gen)
    centers[0] = x[first[0]]
    xc, _ = _centred(x)
    x2 = (xc * xc).sum(1, keepdim=True)
    closest = _sq_dists(xc, xc[first], x2).squeeze(1)
    for c in range(1, k):
        p = closest * w
        total = p.sum()
        # (every point already a centre: fall back to the weights, as sklearn's searchsorted on a flat cumsum would)
        p = torch.where(total > 0, p / total.clamp(min=1e-300), w / w.sum())
        cand = torch.multinomial(p, n_trials, replacement=True, generator=gen)
        d = torch.minimum(_sq_dists(xc, xc[cand], x2), closest[:, None])        # [G, n_trials]
        best = (d * w[:, None]).sum(0).argmin()
        closest = d[:, best]
        centers[c] = x[cand[best]]
    return centers


@torch.no_grad()
def weighted_kmeans(x: torch.Tensor, w: torch.Tensor, k: int, n_init: int = 1, max_iter: int = 300, tol: float = 1e-4,
                    gen: torch.Generator | None = None):
    """weighted k-means on the device (the skeleton step): best of ``n_init`` k-means++ seedings + Lloyd runs (both on centred
    rows).  Returns (centers [k,D] in the coordinates of x, labels int64 [G], inertia)."""
    if gen is None:
        gen = torch.Generator(device=x.device)
        gen.manual_seed(int(np.random.randint(0, 2 ** 31 - 1)))
    best = None
    for _ in range(max(1, n_init)):
        c0 = kmeans_plusplus(x, w, k, gen)
        labels, centers, inertia, _ = lloyd(x, c0, max_iter=max_iter, tol=tol, sample_weight=w)
        if best is None or inertia < best[2]:
            best = (centers, labels, inertia)
    return best


class TooFewReducedPoints(RuntimeError):
    """the point reducer left fewer points than clusters were asked for (the library's RuntimeError, by a name of its own)"""


class RPHKMeans:
    """device-resident ``rph_kmeans.RPHKMeans`` (constructor arguments and fitted attributes as the library's)"""

    def __init__(self, n_clusters=8, n_init=1, w=None, max_point=2000, proj_num=5, max_iter=1000, sample_dist_num=1000,
                 verbose=0, device=None, skeleton_n_init=1):
        self.n_clusters, self.n_init, self.w = n_clusters, n_init, w
        self.skeleton_n_init = skeleton_n_init          # k-means++ restarts of the skeleton step (sklearn's n_init="auto" is 1)
        self.max_point, self.proj_num, self.max_iter, self.sample_dist_num = max_point, proj_num, max_iter, int(sample_dist_num)
        self.verbose = verbose
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("RPHKMeans runs on the GPU; pass device='cpu' explicitly to run the same torch ops on the host")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.inertia_ = self.cluster_centers_ = self.labels_ = self.n_iter_ = self.mean_ = None
        self.reduced_X_ = self.reduced_X_weight_ = self.rp_labels_ = self.rp_iter_ = self.init_centers_ = None

    # -------------------------------------------------------------- point reduction

    def _get_w(self, x: torch.Tensor) -> float:
        if self.w is not None:
            return self.w
        n = x.shape[0]
        a = torch.from_numpy(np.random.choice(n, self.sample_dist_num)).to(x.device)
        b = torch.from_numpy(np.random.choice(n, self.sample_dist_num)).to(x.device)
        # the 2 x 1 000 sampled rows go to the host: numpy's float64 sum, the library's own, gives the same w on every device
        diff = x[a].cpu().numpy().astype(np.float64) - x[b].cpu().numpy().astype(np.float64)
        self.w = float(np.median(np.sqrt((diff ** 2).sum(1))) * 0.5)
        return self.w

    @torch.no_grad()
    def reduce_points(self, x: torch.Tensor):
        """(reduced_X [G,D], weight [G], labels int64 [N] -> row of reduced_X, iterations)"""
        n, dim = x.shape
        w = self._get_w(x)
        if not (w > 0):
            raise RuntimeError("RPH bucket width is zero: the sampled points are all identical")
        labels = torch.arange(n, device=x.device)
        weight = torch.ones(n, dtype=x.dtype, device=x.device)
        red = x
        it = 0
        while it < self.max_iter and red.shape[0] > self.max_point:
            b = np.random.uniform(0, 1, size=(self.proj_num,))
            proj = np.random.normal(0, 1.0 / w, size=(dim, self.proj_num))
            pj = (red.double() @ torch.from_numpy(proj).to(x.device) + torch.from_numpy(b).to(x.device)).to(torch.int32)   # trunc toward 0
            _, bucket = torch.unique(pj, dim=0, return_inverse=True)
            g = int(bucket.max().item()) + 1
            new_w = torch.zeros(g, dtype=x.dtype, device=x.device).index_add_(0, bucket, weight)
            new_x = torch.zeros((g, dim), dtype=x.dtype, device=x.device).index_add_(0, bucket, red * weight[:, None])
            red = new_x / new_w[:, None]
            weight = new_w
            labels = bucket[labels]
            it += 1
        return red, weight, labels, it

    def init_centers(self, x: torch.Tensor):
        """(initial centres, reduced points, their weights, sample -> reduced point, reducer iterations, skeleton inertia,
        skeleton labels) -- the weighted skeleton k-means of rph_kmeans_.py:116-129, on the device"""
        red, weight, labels, it = self.reduce_points(x)
        if red.shape[0] < self.n_clusters:
            raise TooFewReducedPoints("Number of reduced points is too small, please try smaller w or larger proj_num")
        centers, pred, inertia = weighted_kmeans(red, weight, self.n_clusters, n_init=self.skeleton_n_init)
        return centers, red, weight, labels, it, inertia, pred

    # -------------------------------------------------------------- fit

    def fit(self, X):
        x = torch.as_tensor(np.ascontiguousarray(X) if isinstance(X, np.ndarray) else X).to(self.device)
        if x.dtype not in (torch.float32, torch.float64):
            x = x.float()
        self.inertia_ = np.inf
        self.mean_ = _centred(x)[1].cpu().numpy()           # what lloyd takes off the rows: predict takes off the same
        for _ in range(self.n_init):
            centers0, red, weight, rp_labels, rp_iter, _, _ = self.init_centers(x)
            labels, centers, inertia, n_iter = lloyd(x, centers0.to(x))
            if inertia < self.inertia_:
                self.inertia_ = inertia
                self.labels_, self.cluster_centers_, self.n_iter_ = labels.cpu().numpy().astype(np.int32), centers.cpu().numpy(), n_iter
                self.init_centers_, self.reduced_X_, self.reduced_X_weight_ = centers0.cpu().numpy(), red.cpu().numpy(), weight.cpu().numpy()
                self.rp_labels_, self.rp_iter_ = rp_labels.cpu().numpy(), rp_iter
        return self

    def fit_predict(self, X):
        return self.fit(X).labels_

    def predict(self, X):
        """the nearest of ``cluster_centers_``, by the distance step of the fit's last iteration: rows and centres minus the
        column mean of the fitted rows, so that ``predict(X) == labels_`` for the X that was fitted"""
        x = torch.as_tensor(X).to(self.device)
        if x.dtype not in (torch.float32, torch.float64):
            x = x.float()
        xc, m = _centred(x, None if self.mean_ is None else torch.from_numpy(self.mean_).to(self.device).double())
        c = (torch.from_numpy(self.cluster_centers_).to(self.device).double() - m.double()).to(x.dtype)
        return _sq_dists(xc, c).argmin(1).cpu().numpy().astype(np.int32)


def clustering_rph_kmeans(embedding, k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clt = RPHKMeans(n_init=20, n_clusters=k, verbose=0)
        return clt.fit_predict(embedding)


@torch.no_grad()
def clustering_rph_kmeans_sharded(mu_local: torch.Tensor, mu_all, k: int, n_init: int = 20, group=None, device=None):
    """``clustering_rph_kmeans`` with the latent rows sharded over the ranks of ``group``: rank 0, which holds every
    row anyway (it writes latent.npz), reduces the points and seeds the centres exactly as the one-process fit does (same
    numpy draws in the same order); the centres are broadcast (K x 32 floats) and the Lloyd iterations over ALL points --
    rph_kmeans_.py:152-160 -- run on every rank's own rows with the per-iteration all-reduce of ``lloyd(sharded=True)``.
    Returns the labels of all rows in rank order on rank 0 (int32, as the one-process call), None elsewhere."""
    import torch.distributed as dist
    from . import dist as pdist
    me = dist.get_rank(group)
    x = torch.as_tensor(mu_local)
    if device is not None:
        x = x.to(device)
    if x.dtype not in (torch.float32, torch.float64):
        x = x.float()
    clt = None
    if me == 0:
        clt = RPHKMeans(n_init=n_init, n_clusters=k, verbose=0, device=x.device)
        full = torch.as_tensor(mu_all).to(x)
    best = None
    for _ in range(n_init):
        centers0 = clt.init_centers(full)[0].to(x).contiguous() if me == 0 else torch.empty((k, x.shape[1]), dtype=x.dtype, device=x.device)
        if x.is_cuda and dist.get_backend(group) == "gloo":
            h = centers0.cpu()
            dist.broadcast(h, src=0, group=group)
            centers0.copy_(h)
        else:
            dist.broadcast(centers0, src=0, group=group)
        labels, _, inertia, _ = lloyd(x, centers0, group=group, sharded=True)
        if best is None or inertia < best[1]:               # (the inertia is the reduced one: the same choice on every rank)
            best = (labels, inertia)
    got = pdist.gather_rows(best[0].to(torch.int32)[:, None], dst=0, group=group)
    return got[:, 0].cpu().numpy().astype(np.int32) if me == 0 else None


# ---------------------------------------------------------------------------------------------------------------------
# The number of clusters by silhouette score.  The reference's cluster_barcode_reads still carries the parameters of a sweep
# over k (range_step=(4, 100, 3), patience=7, delta=0.0001; clustering.py:70) next to an unused import of sklearn's
# silhouette_score (clustering.py:5): O(N^2) distances per k, hopeless on the host at 10^6 barcodes.  Here the distance sums
# are one HIP kernel (csrc/cluster.hip: pg_cluster_dist_sums), the score a few float64 tensor operations on top of it.

# the torch form of dist_sums works in [query rows, reference rows] tiles of at most 2^20 distances: torch.cdist calls with tens
# of millions of outputs came back partly zero on the MI355X (50 000 x 50 000 rows in blocks of 1 342 x 50 000), small ones agree
# with the kernel and with numpy
_TORCH_FORM_TILE, _TORCH_FORM_ROWS = 1 << 20, 1 << 14


def _as_labels(labels, device) -> torch.Tensor:
    return torch.as_tensor(np.ascontiguousarray(labels) if isinstance(labels, np.ndarray) else labels).to(device=device, dtype=torch.int64)


@torch.no_grad()
def dist_sums(q, x, labels, k: int, n_splits: int = 0) -> torch.Tensor:
    """``S[i, c] = sum over the rows j of x with labels[j] == c of |q_i - x_j|_2``: float64 [n_q, k] on the device of ``x``.

    On the GPU: ``x`` is sorted by label (stable argsort, gathered on the device), the segment starts come from ``bincount``,
    and pg_cluster_dist_sums does the rest on float32 rows -- ``q`` and ``x`` are converted to contiguous float32 when they
    are not (a non-contiguous slice is COPIED, not refused).  ``n_splits``: 0 lets the library cut the reference range so that
    few query rows still fill the device; > 0 forces it (tests).  On a CPU tensor, or with PG_SILHOUETTE_KERNEL=0 (the A/B
    switch), the torch form: tiles of ``torch.cdist`` on float64 copies, formed from the differences, times a one-hot matrix."""
    x = torch.as_tensor(x)
    q = torch.as_tensor(q).to(x.device)
    labels = _as_labels(labels, x.device)
    if q.dim() != 2 or x.dim() != 2 or q.shape[1] != x.shape[1]:
        raise ValueError(f"dist_sums: q {tuple(q.shape)} and x {tuple(x.shape)} are not two matrices of one width")
    if labels.shape != (x.shape[0],):
        raise ValueError(f"dist_sums: {tuple(labels.shape)} labels for {x.shape[0]} rows")
    n_q, n_x = q.shape[0], x.shape[0]
    out = torch.zeros((n_q, k), dtype=torch.float64, device=x.device)
    if n_q == 0 or n_x == 0:
        return out
    if not x.is_cuda or os.environ.get("PG_SILHOUETTE_KERNEL", "1") == "0":
        onehot = torch.zeros((n_x, k), dtype=torch.float64, device=x.device)
        onehot[torch.arange(n_x, device=x.device), labels] = 1.0
        xd, qd = x.double(), q.double()
        x_step = min(n_x, _TORCH_FORM_ROWS)
        q_step = max(1, _TORCH_FORM_TILE // x_step)
        for lo in range(0, n_q, q_step):
            for xlo in range(0, n_x, x_step):
                d = torch.cdist(qd[lo:lo + q_step], xd[xlo:xlo + x_step], compute_mode="donot_use_mm_for_euclid_dist")
                out[lo:lo + q_step] += d @ onehot[xlo:xlo + x_step]
        return out
    from . import _lib
    L = _lib.load()
    order = torch.argsort(labels, stable=True)
    xs = x.to(torch.float32)[order].contiguous()
    qs = q.to(torch.float32).contiguous()
    counts = torch.bincount(labels, minlength=k)            # (refuses negative labels itself)
    if counts.numel() != k:
        raise ValueError(f"dist_sums: labels outside [0, {k})")
    seg = torch.zeros(k + 1, dtype=torch.int64, device=x.device)
    seg[1:] = torch.cumsum(counts, 0)                       # seg[0] = 0, seg[k] = n_x, non-decreasing: what the kernel is promised
    need =_lib.check(L.pg_cluster_dist_sums_workspace_bytes(n_q, n_x, k, n_splits))
    work = torch.empty(need, dtype=torch.uint8, device=x.device) if need else None
    with torch.cuda.device(x.device):
        _lib.check(L.pg_cluster_dist_sums(qs.data_ptr(), n_q, xs.data_ptr(), n_x, x.shape[1], seg.data_ptr(), k, n_splits, out.data_ptr(),
                                          work.data_ptr() if need else None, need, torch.cuda.current_stream().cuda_stream))
    return out


def _checked_labels(x: torch.Tensor, labels, k: int):
    """(labels int64 on the device of x, cluster sizes int64 [k]) after the refusals of the silhouette"""
    if k < 2:
        raise ValueError(f"silhouette: k = {k}, at least 2 clusters are needed")
    labels = _as_labels(labels, x.device)
    if labels.shape != (x.shape[0],):
        raise ValueError(f"silhouette: {tuple(labels.shape)} labels for {x.shape[0]} rows")
    if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= k):
        raise ValueError(f"silhouette: labels outside [0, {k})")
    counts = torch.bincount(labels, minlength=k)
    if int((counts > 0).sum()) < 2:
        raise ValueError("silhouette: fewer than two non-empty clusters")
    return labels, counts


@torch.no_grad()
def silhouette_samples(x, labels, k: int, rows=None) -> torch.Tensor:
    """the silhouette coefficient of every row (or of ``rows``, indices into x) as scikit-learn defines it: with
    ``S = dist_sums(.)``, ``a_i = S[i, own] / (n_own - 1)``, ``b_i = min over the other non-empty clusters of S[i, c] / n_c``,
    ``s_i = (b_i - a_i) / max(a_i, b_i)``, and 0 for the only row of its cluster or where the quotient is not finite.
    ``rows`` restricts the QUERY side only: the distances still run to all rows of x and the cluster sizes are those of all
    rows, so every s_i is exact (scikit-learn's ``sample_size`` thins both sides instead).  float64 on the device of x."""
    x = torch.as_tensor(x)
    labels, counts = _checked_labels(x, labels, k)
    if rows is None:
        q, own = x, labels
    else:
        rows = torch.as_tensor(rows).to(device=x.device, dtype=torch.int64)
        q, own = x[rows], labels[rows]
    s = dist_sums(q, x, labels, k)
    n_own = counts[own]
    a = s.gather(1, own[:, None]).squeeze(1) / (n_own - 1).clamp(min=1).double()
    other = s / counts.double()[None, :]                                    # (an empty cluster: 0 / 0, masked next)
    other.masked_fill_((counts == 0)[None, :], float("inf"))
    other.scatter_(1, own[:, None], float("inf"))
    b = other.min(dim=1).values
    sil = (b - a) / torch.maximum(a, b)
    return torch.where((n_own > 1) & torch.isfinite(sil), sil, torch.zeros_like(sil))


def _sample_rows(n: int, sample, seed: int):
    """``sample`` distinct rows of n, sorted, from a generator of its own (numpy's global one, whose order the RPH draws depend
    on, is never touched); None when that is all rows"""
    if sample is None or sample >= n:
        return None
    return np.sort(np.random.RandomState(seed).choice(n, int(sample), replace=False))


def silhouette_score(x, labels, k: int, sample=None, seed: int = 0) -> float:
    """the mean silhouette coefficient; with ``sample`` < N the mean over that many rows drawn by ``RandomState(seed)`` --
    an unbiased estimate, every term exact (see silhouette_samples)"""
    x = torch.as_tensor(x)
    return float(silhouette_samples(x, labels, k, rows=_sample_rows(x.shape[0], sample, seed)).mean())


def choose_clusters(embedding, range_step=(4, 100, 3), patience=7, delta=1e-4, sweep_n_init=5, sample=16384, seed=0, device=None):
    """the number of clusters by silhouette score: ``(best_k, table)``.  Visits k in ``range(*range_step)`` (no further than
    N - 1), fits ``RPHKMeans(n_clusters=k, n_init=sweep_n_init)`` to the embedding -- copied to the device once -- and scores the
    fit on the same ``sample`` rows every time.  A k becomes the best when its score exceeds the best so far by more than
    ``delta``; after ``patience`` consecutive k without that the sweep ends.  ``table``: ``(k, score, inertia, n_nonempty)``
    per visited k; a fit with fewer than two non-empty clusters scores -1; a k for which the point reducer leaves fewer than k
    points (TooFewReducedPoints) ends the sweep like patience does.  The defaults are the reference's
    (cluster_barcode_reads, clustering.py:70).  The fits draw from numpy's global generator as every RPHKMeans does; its
    state is put back at the end, so that whatever follows draws what it would have drawn without the sweep."""
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("choose_clusters runs on the GPU; pass device='cpu' explicitly to run the same torch ops on the host")
        device = torch.device("cuda", torch.cuda.current_device())
    x = torch.as_tensor(np.ascontiguousarray(embedding) if isinstance(embedding, np.ndarray) else embedding).to(device)
    if x.dtype not in (torch.float32, torch.float64):
        x = x.float()
    n = x.shape[0]
    if n < 6:
        raise ValueError(f"choose_clusters: {n} rows, at least 6 are needed")
    rows = _sample_rows(n, sample, seed)
    table, best_k, best, stale = [], None, -np.inf, 0
    state = np.random.get_state()
    try:
        for k in range(*range_step):
            if k > n - 1:
                break
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    clt = RPHKMeans(n_clusters=k, n_init=sweep_n_init, verbose=0, device=device).fit(x)
            except TooFewReducedPoints:
                # the rows collapse onto fewer than k reduced points (tight, well separated groups): this k cannot be fitted,
                # larger ones neither -- the sweep ends here with what it has, unless it has nothing
                if best_k is None:
                    raise
                logging.info(f"silhouette sweep: fewer than {k} reduced points, stopping at k = {table[-1][0]}")
                break
            labels =torch.from_numpy(clt.labels_.astype(np.int64)).to(device)
            nonempty = int((torch.bincount(labels, minlength=k) > 0).sum())
            score = float(silhouette_samples(x, labels, k, rows=rows).mean()) if nonempty >= 2 else -1.0
            table.append((k, score, float(clt.inertia_), nonempty))
            if score > best + delta:
                best_k, best, stale = k, score, 0
            else:
                stale += 1
                if stale >= patience:
                    break
    finally:
        np.random.set_state(state)
    if best_k is None:
        raise ValueError(f"choose_clusters: range_step = {tuple(range_step)} holds no k in [2, {n - 1}]")
    return best_k, table


def write_silhouette_tsv(path: str, table) -> None:
    with open(path, "w") as tsv:
        tsv.write("k\tscore\tinertia\tclusters\n")
        for k, score, inertia, nonempty in table:
            tsv.write("%d\t%.6f\t%.6f\t%d\n" % (k, score, inertia, nonempty))


def write_clusters_tsv(path: str, clusters, barcodes) -> None:
    """``<label>\\t<bc1>,<bc2>,...`` per label in first-seen order (clustering.py:107-112)"""
    cluster2barcodes = defaultdict(list)
    for lab, bc in zip(clusters, barcodes):
        cluster2barcodes[lab].append(str(bc))
    with open(path, "w") as tsv:
        for cluster_id in cluster2barcodes:
            tsv.write("{}\t{}\n".format(cluster_id, ",".join(cluster2barcodes[cluster_id])))


def cluster_barcode_reads(args, model_path, cluster_path, script_path, clusters=None, device=None):
    """step 3 of pangaea.py: latent.npz/barcodes.npz -> clusters.npz, clusters.tsv, cluster_bin<label>.{fq,barcode},
    clustering_finished -- the on-disk bin layout the unchanged reassembly stage reads (bin_assembly.sh:18).
    ``clusters``: labels already computed for the rows of latent.npz (the sharded Lloyd of a multi-rank run).
    Without ``args.clusters``: ``args.auto_clusters == "silhouette"`` picks the number by the silhouette sweep over
    ``args.cluster_range`` (choose_clusters; its table goes to silhouette.tsv), anything else asks the reference's metaphlan
    script.  ``device``: where the sweep and the fit run when not on the current GPU."""
    from .binwriter import extract_reads
    output_npz = os.path.join(cluster_path, "clusters.npz")
    output_tsv = os.path.join(cluster_path, "clusters.tsv")
    embedding_path = os.path.join(model_path, "latent.npz")
    barcodes_path = os.path.join(model_path, "barcodes.npz")
    if not os.path.isfile(embedding_path) or not os.path.isfile(barcodes_path):
        raise FileNotFoundError(f"{embedding_path} or {barcodes_path} not found")
    if not os.path.isfile(output_tsv) and clusters is not None:
        barcodes = np.load(barcodes_path)["arr_0"]
        assert len(clusters) == len(barcodes)
        np.savez(output_npz, clusters)
        logging.info("saving clustering tsv")
        write_clusters_tsv(output_tsv, clusters, barcodes)
    elif not os.path.isfile(output_tsv):
        embedding = np.load(embedding_path)["arr_0"]
        barcodes = np.load(barcodes_path)["arr_0"]
        if args.clusters:
            num_classes = args.clusters
        elif getattr(args, "auto_clusters", "metaphlan") == "silhouette":
            # no external profiler: the sweep the reference's signature still describes, scored on the GPU (choose_clusters)
            spec = getattr(args, "cluster_range", None) or "4,100,3"
            range_step = tuple(int(v) for v in spec.split(",")) if isinstance(spec, str) else tuple(spec)
            if len(range_step) != 3 or range_step[2] < 1:
                raise ValueError(f"--cluster_range {spec!r}: LO,HI,STEP with STEP >= 1 expected")
            num_classes, table = choose_clusters(embedding, range_step=range_step, device=device)
            write_silhouette_tsv(os.path.join(cluster_path, "silhouette.tsv"), table)
            logging.info(f"estimated num_classes: {num_classes}")
        else:
            # the reference estimates 8 x Shannon diversity with metaphlan (clustering.py:92-102): an external tool,
            # outside this path -- run the reference's own script when it is installed next to us
            diversity = os.path.join(script_path, "scripts", "calculate_diversity.sh")
            if not os.path.isfile(diversity):
                raise FileNotFoundError("number of clusters (-c) not given and scripts/calculate_diversity.sh not found")
            reads = args.reads1 if (args.reads1 and args.reads2) else args.interleaved_reads
            run_cmd([diversity, reads, args.metaphlan_db, cluster_path])
            shannon = np.loadtxt(os.path.join(cluster_path, "metaphlan_tmp/diversity_analysis/profiles_table_shannon.txt"))
            num_classes = int(8 * shannon)
            logging.info(f"estimated num_classes: {num_classes}")
            run_cmd(["rm", "-rf", os.path.join(cluster_path, "metaphlan_tmp")])
        if device is None:
            clusters = clustering_rph_kmeans(embedding, num_classes)
        else:                                               # (the same call on a named device: the host tests)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                clusters = RPHKMeans(n_init=20, n_clusters=num_classes, verbose=0, device=device).fit_predict(embedding)
        np.savez(output_npz, clusters)
        logging.info("saving clustering tsv")
        write_clusters_tsv(output_tsv, clusters, barcodes)
    else:
        logging.info("existing clustering result found")
    prefix = os.path.join(cluster_path, "cluster")
    if args.reads1 and args.reads2:
        extract_reads(args.reads1, args.reads2, output_tsv, prefix)
    elif args.interleaved_reads:
        extract_reads(args.interleaved_reads, None, output_tsv, prefix)
    else:
        logging.error("no reads provided")
        raise FileNotFoundError("no reads provided")
    with open(os.path.join(cluster_path, "clustering_finished"), "w") as f:
        f.write("finished")
