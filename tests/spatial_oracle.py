"""numpy oracle of the spatial statistics of dims_autocorr: the self-kNN graph by brute force and Moran's I in fp64.

The graph ranks by (d^2, index), d^2 as sklearn forms it: coordinates in fp64, each (x_k - y_k)^2 rounded on its own,
the terms added in coordinate order (numpy's element-wise operations do not fuse).  Moran's I as squidpy's
spatial_autocorr(mode="moran") with row-normalised weights; the mean is taken around the column's first value, as the
library does, so a constant column gives NaN exactly."""
from __future__ import annotations

import numpy as np


def knn_rows(X, K, rows=None, block=64):
    """(len(rows), K) int64: for each row i, the K other points nearest to point i, ascending by (d^2, index)."""
    X = np.asarray(X, dtype=np.float64)
    N, d = X.shape
    rows = np.arange(N) if rows is None else np.asarray(rows, dtype=np.int64)
    out = np.empty((len(rows), K), dtype=np.int64)
    for b0 in range(0, len(rows), block):
        r = rows[b0:b0 + block]
        d2 = (X[None, :, 0] - X[r, None, 0]) ** 2
        for k in range(1, d):
            d2 = d2 + (X[None, :, k] - X[r, None, k]) ** 2
        d2[np.arange(len(r)), r] = np.inf
        kth = np.partition(d2, K - 1, axis=1)[:, K - 1]
        for a, i in enumerate(r):
            cand = np.nonzero(d2[a] <= kth[a])[0]
            cand = cand[cand != i]
            o = np.lexsort((cand, d2[a, cand]))
            out[b0 + a] = cand[o[:K]]
    return out


def morans_i(values, nbr):
    """(L,) float64 Moran's I of every column of values (N,L) over the neighbour table nbr (N,K), weights 1/K."""
    V = np.asarray(values, dtype=np.float64)
    nbr = np.asarray(nbr)
    mean = V[0] + (V - V[0]).sum(axis=0) / V.shape[0]
    z = V - mean
    lag = z[nbr].mean(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (z * lag).sum(axis=0) / (z * z).sum(axis=0)
