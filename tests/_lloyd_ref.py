"""Plain numpy float64 restatements of the two loops of step 3 (pangaea_amd/clustering.py): Lloyd's iterations with
scikit-learn's semantics (``KMeans(init=centres, n_init=1)``, the call the reference ends in, rph_kmeans_.py:152-160) and one
round of the RPH point reducer (point_reducer_cy.py:47-76, _point_reducer_cy_lib.cpp:5-28).  Written to be read, not to be
fast: distances come from the differences, never from |x|^2 - 2 x.c + |c|^2, and every sum is float64.

``lloyd_ref`` also reports the MARGIN of the trajectory it walked -- how far the closest decision of any E-step was from a tie,
relative to the size of the numbers a float32 distance step has to subtract.  A test that demands equal labels and equal
iteration counts from a float32 implementation asserts that margin first; without it the demand would be unfair."""
import numpy as np


def sq_dists(X, C):
    """[n, k] squared distances from the differences, float64 (one centre at a time: no n x k x dim temporary)"""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    d = np.empty((X.shape[0], C.shape[0]))
    for j in range(C.shape[0]):
        d[:, j] = ((X - C[j]) ** 2).sum(1)
    return d


def _margin(d, lab, xn, cn):
    """min over the rows and the centres j != best of (d_j - d_best) / ((|x'| + |c'_j|)^2 + (|x'| + |c'_best|)^2): the two
    competing centres only, so that a centre far out does not shrink the margin of the others; an exact 0 / 0 is a tie: 0"""
    n, k = d.shape
    if k < 2 or n == 0:
        return np.inf
    rows = np.arange(n)
    size = (xn[:, None] + cn[None, :]) ** 2
    den = size + size[rows, lab][:, None]
    num = d - d[rows, lab][:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(den > 0, num / den, 0.0)
    ratio[rows, lab] = np.inf
    return float(ratio.min())


def lloyd_ref(X, init, w=None, max_iter=300, tol=1e-4):
    """(labels, centres, inertia, n_iter, gap) of scikit-learn's Lloyd from the start centres ``init``:
      * the column mean of X is subtracted first (and added back to the centres at the end);
      * E-step: nearest centre by ((x - c)**2).sum(), the first of equals;
      * M-step: weighted sums; a cluster of weight 0 takes the point farthest from its own centre -- the points in descending
        order of that distance (stable), one per empty cluster in index order -- and the cluster that point leaves loses it
        (its sum, its weight and its label).  A cluster whose weight is still 0 after that (the point it took has weight 0,
        which scikit-learn handles by another route; no caller here passes such weights) sits on the column mean;
      * stop when the labels repeat, or when the squared centre shift is <= tol x the mean column variance;
      * one more E-step gives the labels and the inertia that are returned.
    ``gap``: the margin (see _margin) of the closest decision of ANY of those E-steps, in centred coordinates."""
    X = np.asarray(X, dtype=np.float64)
    C = np.array(init, dtype=np.float64)
    n, dim = X.shape
    k = C.shape[0]
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    mean = X.mean(0)
    Xc = X - mean
    C = C - mean
    tol_abs = tol * float(Xc.var(0).mean())
    xn = np.sqrt((Xc ** 2).sum(1))
    rows = np.arange(n)
    gap = np.inf
    lab_old = None
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        d = sq_dists(Xc, C)
        lab = d.argmin(1)
        gap = min(gap, _margin(d, lab, xn, np.sqrt((C ** 2).sum(1))))
        mind = d[rows, lab]
        sums = np.zeros((k, dim))
        np.add.at(sums, lab, Xc * w[:, None])
        cnt = np.bincount(lab, weights=w, minlength=k)
        empty = np.nonzero(cnt == 0)[0]
        if empty.size:
            far = np.argsort(-mind, kind="stable")[:empty.size]
            for e, f in zip(empty, far):
                old = lab[f]
                sums[old] -= Xc[f] * w[f]
                cnt[old] -= w[f]
                sums[e] = Xc[f] * w[f]
                cnt[e] = w[f]
                lab[f] = e
        new = np.where(cnt[:, None] > 0, sums / np.where(cnt > 0, cnt, 1.0)[:, None], 0.0)
        shift = float(((new - C) ** 2).sum())
        C = new
        if lab_old is not None and np.array_equal(lab, lab_old):
            break
        lab_old = lab
        if shift <= tol_abs:
            break
    d = sq_dists(Xc, C)
    lab = d.argmin(1)
    gap = min(gap, _margin(d, lab, xn, np.sqrt((C ** 2).sum(1))))
    inertia = float((w * d[rows, lab]).sum())
    return lab, C + mean, inertia, n_iter, gap


def first_seen(labels):
    """a partition in canonical form: every label replaced by the rank of its first occurrence"""
    labels = np.asarray(labels)
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv.ravel()]


def reduce_round_ref(red, weight, w, b, proj, rounding=np.trunc):
    """one round of the point reducer: the rows of ``red`` (weights ``weight``) whose ``proj.shape[1]`` integers
    ``rounding(red @ proj + b)`` all agree are merged into their weighted mean.  ``proj`` was drawn N(0, 1/w) by the caller, in
    the reducer's order; ``w`` is the bucket width it was drawn with (positive, or the reducer refuses).  The library truncates
    toward zero (a C cast); ``rounding=np.floor`` gives the partition a floor would, for tests that pin the difference.
    Returns (partition [n] in first-seen form, weights [G], float64 weighted means [G, dim], edge), buckets numbered by first
    occurrence; ``edge`` is the smallest distance of any projection to an integer: how far the partition is from changing."""
    if not (w > 0):
        raise RuntimeError("bucket width is zero")
    red = np.asarray(red).astype(np.float64)
    weight = np.asarray(weight, dtype=np.float64)
    p = red @ np.asarray(proj, dtype=np.float64) + np.asarray(b, dtype=np.float64)
    edge = float(np.abs(p - np.round(p)).min())
    _, inv = np.unique(rounding(p), axis=0, return_inverse=True)
    part = first_seen(inv)
    g = int(part.max()) + 1
    new_w = np.bincount(part, weights=weight, minlength=g)
    sums = np.zeros((g, red.shape[1]))
    np.add.at(sums, part, red * weight[:, None])
    return part, new_w, sums / new_w[:, None], edge
