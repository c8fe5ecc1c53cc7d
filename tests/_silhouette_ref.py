"""The silhouette in plain numpy float64, restated from its definition: distances from the differences, a loop over the
clusters, nothing shared with pangaea_amd.  O(N^2): keep N <= 2 000."""
import numpy as np


def dist_sums(q, x, labels, k):
    """S[i, c] = sum over the rows j of x with labels[j] == c of |q_i - x_j|_2, float64 [n_q, k]"""
    q = np.asarray(q, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    out = np.zeros((q.shape[0], k), dtype=np.float64)
    for c in range(k):
        members = x[labels == c]
        if not len(members):
            continue
        for lo in range(0, q.shape[0], 64):                    # (blocks of query rows: the differences of a block fit in memory)
            diff = q[lo:lo + 64, None, :] - members[None, :, :]
            out[lo:lo + 64, c] = np.sqrt((diff * diff).sum(axis=2)).sum(axis=1)
    return out


def silhouette_samples(x, labels, k, rows=None):
    """s_i of every row (or of ``rows``) against ALL rows of x: a = mean distance to the other rows of the own cluster,
    b = the smallest mean distance to another non-empty cluster, s = (b - a) / max(a, b); 0 for a singleton or 0 / 0"""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    rows = np.arange(len(x)) if rows is None else np.asarray(rows)
    counts = np.array([(labels == c).sum() for c in range(k)])
    s = dist_sums(x[rows], x, labels, k)
    out = np.zeros(len(rows), dtype=np.float64)
    for n, i in enumerate(rows):
        own = labels[i]
        if counts[own] == 1:
            continue
        a = s[n, own] / (counts[own] - 1)
        b = min(s[n, c] / counts[c] for c in range(k) if c != own and counts[c] > 0)
        if max(a, b) > 0:
            out[n] = (b - a) / max(a, b)
    return out


def silhouette_score(x, labels, k, rows=None):
    return float(silhouette_samples(x, labels, k, rows).mean())
