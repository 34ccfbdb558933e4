"""numpy oracle of the exact K-nearest mean behind smooth_spatial_factors (gpz_knn_mean), by brute force.

For each query the keys (d^2, index) of the points up to the K-th distance are sorted (``lexsort``) and the first K
taken: exact ties go to the lower index.  d^2 as sklearn forms it: coordinates in fp64, each (x_k - z_k)^2 rounded on its own, the terms added in
coordinate order (numpy's element-wise operations do not fuse).  The set is returned in ascending index order, the
mean is numpy's fp64 mean over it."""
from __future__ import annotations

import numpy as np


def knn_sets(X, Z, K, rows=None, block=32):
    """(len(rows), K) int64: for each query Z[r] the K points of X nearest to it, in ascending index order."""
    X = np.asarray(X, dtype=np.float64)
    Z = np.asarray(Z, dtype=np.float64)
    rows = np.arange(len(Z)) if rows is None else np.asarray(rows, dtype=np.int64)
    index = np.arange(len(X))
    out = np.empty((len(rows), K), dtype=np.int64)
    for b0 in range(0, len(rows), block):
        r = rows[b0:b0 + block]
        d2 = (X[None, :, 0] - Z[r, None, 0]) ** 2
        for k in range(1, X.shape[1]):
            d2 = d2 + (X[None, :, k] - Z[r, None, k]) ** 2
        kth = np.partition(d2, K - 1, axis=1)[:, K - 1]          # only keys up to the K-th distance need sorting
        for a in range(len(r)):
            cand = index[d2[a] <= kth[a]]
            out[b0 + a] = np.sort(cand[np.lexsort((cand, d2[a, cand]))[:K]])
    return out


def knn_mean(X, F, Z, K, rows=None):
    """(len(rows), L) float64: the mean of F over each query's set; also returns the sets."""
    sets = knn_sets(X, Z, K, rows)
    return np.asarray(F, dtype=np.float64)[sets].mean(axis=1), sets
