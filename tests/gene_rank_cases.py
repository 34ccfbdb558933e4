"""Seeded cases and fp64 numpy oracles for the per-gene scores of gpzoo_amd/csrc/gene_rank.hip (gene deviance, Moran's I of
every gene) and the graph moments of ``utilities.gene_autocorr``.  Everything here runs on the CPU.

Counts (D = 37 genes, N spots) depend on N alone, the neighbour table on (N, K).  Gene rows, by index (``ROW_KINDS``):

  empty        no stored entry                                  one         a single entry
  every        a count at every spot                            constant    the same count at every spot
  g-1, g, g+1  that many entries for the plan's granularity g   mutual      entries at the spots 0 and 1 only, which name
                                                                            each other in every table
  unnamed      entries only at the last spots, which no row of the table names (every table but the complete one at N = 7, K = 6)
  the rest     Poisson counts with rates 0.002 ... 400, log-spaced

The variant "holes" is the same array with three spots emptied (spots with no counts at all; rows ``every`` and
``constant`` then miss those spots).  Rows that do not fit N (g + 1 > N) are Poisson rows."""
from __future__ import annotations

import functools

import numpy as np

import spatial_oracle as SO

D = 37
NS = (7, 257, 1037, 4099)
KS = (1, 6, 32)
GRAPHS = [(N, K) for N in NS for K in KS if K < N]           # N = 7 runs with K = 1 and 6
VARIANTS = ("full", "holes")
UNNAMED = 3                                     # the last UNNAMED spots are named by no row, where the table leaves room
MORAN_ATOL = 1e-10                              # the bound of tests/test_hip_spatial_autocorr.py for the dense kernel
DEVIANCE_RTOL = 1e-11                           # x scale_d: fp64 epsilon x 4099 sequential terms (4.5e-13), ~20x for the device's log


def granularity() -> int:
    """Stored entries of a gene row per sweep of its workgroup: the plan query's gene_chunk (host only)."""
    from gpzoo_amd import ops
    g = ops.gene_rank_plan(NS[-1], D, 1)["gene_chunk"]
    assert g == ops.gene_rank_plan(NS[-1], D, 1, K=6)["gene_chunk"]
    return g


def row_kinds(N: int) -> dict:
    g = granularity()
    kinds = {"empty": 0, "one": 1, "every": 2, "constant": 3, "mutual": 7, "unnamed": 8}
    for j, n in enumerate((g - 1, g, g + 1)):
        if n <= N:
            kinds[f"g{n - g:+d}"] = 4 + j
    return kinds


def holes(N: int):
    return np.array([2, N // 2, N - 4]) if N > 7 else np.array([3])


@functools.lru_cache(maxsize=None)
def counts(N: int, variant: str = "full") -> np.ndarray:
    """(D, N) float32 counts (exact in fp32)."""
    rng = np.random.default_rng(1000 + N)
    rates = np.exp(np.linspace(np.log(0.002), np.log(400.0), D))
    Y = rng.poisson(rates[:, None] * rng.uniform(0.5, 1.5, size=(1, N)), size=(D, N)).astype(np.float64)
    Y[D - 1] = np.maximum(Y[D - 1], 1.0)                     # every spot has counts before the holes are cut
    g = granularity()
    kinds = row_kinds(N)
    Y[kinds["empty"]] = 0
    Y[kinds["one"]] = 0
    Y[kinds["one"], N // 2 + 1] = 3
    Y[kinds["every"]] = rng.integers(1, 40, N)
    Y[kinds["constant"]] = 5
    for name, n in (("g-1", g - 1), ("g+0", g), ("g+1", g + 1)):
        if name in kinds:
            Y[kinds[name]] = 0
            Y[kinds[name], rng.choice(N, n, replace=False)] = rng.integers(1, 9, n)
    Y[kinds["mutual"]] = 0
    Y[kinds["mutual"], :2] = (4, 7)
    Y[kinds["unnamed"]] = 0
    Y[kinds["unnamed"], N - UNNAMED:] = (2, 9, 1)
    if variant == "holes":
        Y[:, holes(N)] = 0
    else:
        assert variant == "full"
    out = Y.astype(np.float32)
    assert (out == Y).all()
    out.setflags(write=False)
    return out


def n_unnamed(N: int, K: int) -> int:
    return max(0, min(UNNAMED, N - 1 - K))


@functools.lru_cache(maxsize=None)
def graph(N: int, K: int) -> np.ndarray:
    """(N, K) int64: K distinct neighbours per row, no self edge; rows 0 and 1 name each other; the last n_unnamed(N, K)
    spots are named by nobody."""
    rng = np.random.default_rng(7 * N + K)
    pool = N - n_unnamed(N, K)
    nbr = np.empty((N, K), dtype=np.int64)
    for i in range(N):
        pick = rng.choice(pool, K + 1, replace=False)
        nbr[i] = pick[pick != i][:K]
    for a, b in ((0, 1), (1, 0)):
        if b not in nbr[a]:
            nbr[a, 0] = b
    nbr.setflags(write=False)
    return nbr


def log_values(N: int, variant: str):
    """``log_normalize(counts, center=False)`` of the case on the CPU: the SparseExpression and its dense (D, N) fp32 array."""
    import torch
    from gpzoo_amd.likelihoods import SparseCounts
    from gpzoo_amd.utilities import log_normalize
    e = log_normalize(SparseCounts(torch.tensor(counts(N, variant))), center=False)
    return e, e.values.to_dense().numpy()


# ---- oracles ---------------------------------------------------------------------------------------------------------

def moran_oracle(dense, nbr):
    """(D,) Moran's I of every gene of dense (D, N): the project's oracle on the dense transpose, zeros included."""
    return SO.morans_i(np.asarray(dense, dtype=np.float64).T, nbr)


def moran_expanded(dense, nbr):
    """The expanded form the kernel evaluates, in numpy with sequential fp64 sums over the stored entries (np.cumsum adds in
    order), every product and sum rounded on its own."""
    X = np.asarray(dense, dtype=np.float64)
    Dn, N = X.shape
    K = nbr.shape[1]
    indeg = np.bincount(nbr.reshape(-1), minlength=N).astype(np.float64)
    out = np.full(Dn, np.nan)
    for d in range(Dn):
        nz = np.nonzero(X[d])[0]
        if nz.size == 0:
            continue
        x = X[d, nz]
        if nz.size == N and x.min() == x.max():
            continue
        lag = np.cumsum(X[d][nbr[nz]], axis=1)[:, -1]
        S, Q, C, A = (np.cumsum(v)[-1] for v in (x, x * x, x * lag, indeg[nz] * x))
        xbar = S / N
        den = K * (Q - N * (xbar * xbar))
        if den > 0:
            out[d] = (C - xbar * (K * S + A) + N * K * (xbar * xbar)) / den
    return out


def moments_oracle(nbr):
    """(expected, variance) of Moran's I under normality from the dense row-normalised W, as squidpy / libpysal form them."""
    N, K = nbr.shape
    W = np.zeros((N, N))
    W[np.arange(N)[:, None], nbr] = 1.0 / K
    S0 = W.sum()
    S1 = 0.5 * ((W + W.T) ** 2).sum()
    S2 = ((W.sum(axis=1) + W.sum(axis=0)) ** 2).sum()
    EI = -1.0 / (N - 1)
    VI = (N * N * S1 - N * S2 + 3.0 * S0 * S0) / ((N * N - 1.0) * S0 * S0) - EI * EI
    return EI, VI


def moments_bound(N, K, VI):
    """|variance - oracle| allowed: 1e-12 relative.  Over the complete graph (K = N - 1) Moran's I is -1 / (N - 1) whatever
    the values, its variance is exactly 0 and both sides are the rounding of terms of size 1 / (N - 1)^2: 1e-15 absolute."""
    return 1e-15 if K == N - 1 else 1e-12 * abs(VI)


def deviance_oracle(dense, size, family):
    """dict(sum, count, deviance, scale), each (D,): elementwise on the dense array, 0 for 0 log 0.  ``scale`` is
    2 (sum |saturated terms| + |null terms|), what the GPU test's bound is relative to."""
    Y = np.asarray(dense, dtype=np.float64)
    size = np.asarray(size, dtype=np.float64)
    S = size.sum()
    s = Y.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        sat = np.where(Y > 0, Y * np.log(Y / size), 0.0)
        if family == "binomial":
            sat = sat + np.where((Y > 0) & (size > Y), (size - Y) * np.log1p(-Y / size), 0.0)
        p = s / S
        if family == "poisson":
            null = [np.where(s > 0, s * np.log(p), 0.0)]
        else:
            assert family == "binomial"
            ok = (s > 0) & (p < 1)
            l1 = np.where(ok, np.log1p(-np.where(ok, p, 0.0)), 0.0)
            null = [np.where(ok, s * (np.log(p) - l1), 0.0), np.where(ok, S * l1, 0.0)]
    count = (Y != 0).sum(axis=1).astype(np.float64)
    dev = np.where(count > 0, 2.0 * (sat.sum(axis=1) - sum(null)), 0.0)
    scale = 2.0 * (np.abs(sat).sum(axis=1) + sum(np.abs(t) for t in null))
    return dict(sum=s, count=count, deviance=dev, scale=scale)


def sizes(N: int, variant: str, which: str) -> np.ndarray:
    """(N,) fp64 sizes: "totals" = the spots' total counts (0 at an emptied spot, which has no stored entry), or "factors" =
    seeded positive values."""
    if which == "totals":
        return counts(N, variant).astype(np.float64).sum(axis=0)
    assert which == "factors"
    return np.random.default_rng(50 + N).uniform(0.25, 4.0, N)
