"""Seeded cases and fp64 / integer oracles for the permutation null of Moran's I (gpzoo_amd/csrc/moran_perm.hip,
``utilities.gene_autocorr(n_perms=)``).  TEST INFRASTRUCTURE ONLY; numpy, everything runs on the CPU.

The data are those of tests/gene_rank_cases.py: D = 37 genes with its row kinds (empty, one entry, every spot, constant, the
three chunk-boundary rows, mutual pair, unnamed spots), N in NS, the neighbour tables of GRAPHS.  Two fixtures per (N, K):

  "counts"  the integer counts, variant "holes": comparisons of the statistic are exact, ties included
  "log"     log_normalize(counts, center=False), variant "full": non-integer values

and P = 19 permutations per N from np.random.default_rng(5 + N).  A permutation pi turns gene x into x^pi[i] = x[pi[i]].
N = 7, K = 6 is the complete graph: every permutation gives the same I (kept on purpose: n_ge = n_le = P exactly)."""
from __future__ import annotations

import functools

import numpy as np

import gene_rank_cases as G

P = 19
FIXTURES = {"counts": "holes", "log": "full"}
BAND = 2.0 * G.MORAN_ATOL          # |I_pi - I| of two values each within MORAN_ATOL of its oracle
BAND_SHARE_MAX = 0.05              # of the (gene, permutation) pairs of a "log" fixture with N >= 257


@functools.lru_cache(maxsize=None)
def perms(N: int) -> np.ndarray:
    """(P, N) int32 permutations."""
    rng = np.random.default_rng(5 + N)
    out = np.stack([rng.permutation(N) for _ in range(P)]).astype(np.int32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dense(N: int, kind: str) -> np.ndarray:
    """(D, N) float32 values of the fixture."""
    if kind == "counts":
        return G.counts(N, FIXTURES[kind])
    out = G.log_values(N, FIXTURES[kind])[1]
    out.setflags(write=False)
    return out


def relabelled(nbr, pi):
    """T_pi[pi[i], m] = pi[nbr[i, m]]: the table under which the unpermuted gene scores what x^pi scores under nbr."""
    pi = np.asarray(pi, dtype=np.int64)
    T = np.empty_like(nbr)
    T[pi] = pi[nbr]
    return T


@functools.lru_cache(maxsize=None)
def sims_oracle(N: int, K: int, kind: str) -> np.ndarray:
    """(D, P) fp64: the project's Moran oracle on the permuted dense array, per permutation."""
    X, nbr = dense(N, kind), G.graph(N, K)
    out = np.stack([G.moran_oracle(X[:, pi], nbr) for pi in perms(N)], axis=1)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def observed_oracle(N: int, K: int, kind: str) -> np.ndarray:
    out = G.moran_oracle(dense(N, kind), G.graph(N, K))
    out.setflags(write=False)
    return out


def _order_statistic(X, nbr, indeg):
    """Per gene, N C - S A in Python integers (X int64 (D, N))."""
    N = X.shape[1]
    C = (X * X[:, nbr].sum(axis=2)).sum(axis=1)
    A = (X * indeg).sum(axis=1)
    S = X.sum(axis=1)
    return [N * int(c) - int(s) * int(a) for c, s, a in zip(C, S, A)]


@functools.lru_cache(maxsize=None)
def counts_oracle_exact(N: int, K: int):
    """(n_ge, n_le), int64 (D,): the permutations with I_pi >= I and I_pi <= I for the integer "counts" fixture, decided on
    N C - S A in integers (the denominator of I does not depend on pi).  A gene without I (N Q - S^2 = 0: no entry, or one
    value at every spot) counts nothing."""
    Y = dense(N, "counts")
    X = Y.astype(np.int64)
    assert (X == Y).all()
    nbr = G.graph(N, K)
    indeg = np.bincount(nbr.reshape(-1), minlength=N).astype(np.int64)
    t0 = _order_statistic(X, nbr, indeg)
    scored = [N * int(q) - int(s) ** 2 > 0 for q, s in zip((X * X).sum(axis=1), X.sum(axis=1))]
    n_ge, n_le = np.zeros(G.D, dtype=np.int64), np.zeros(G.D, dtype=np.int64)
    for pi in perms(N):
        t = _order_statistic(X[:, pi], nbr, indeg)
        for d in range(G.D):
            if scored[d]:
                n_ge[d] += t[d] >= t0[d]
                n_le[d] += t[d] <= t0[d]
    return n_ge, n_le


def counts_bracket(N: int, K: int, kind: str):
    """(ge, le, band), int64 (D,) each, from the fp64 oracles: the permutations definitely above (I_pi > I + BAND) and
    definitely below (I_pi < I - BAND), and those inside the band, which may count either way.  A correct n_ge lies in
    [ge, ge + band], n_le in [le, le + band]; all zero for a gene without I."""
    I, sims = observed_oracle(N, K, kind), sims_oracle(N, K, kind)
    ok = ~np.isnan(I)
    assert (np.isnan(sims) == ~ok[:, None]).all()
    with np.errstate(invalid="ignore"):
        diff = sims - I[:, None]
        ge = (ok[:, None] & (diff > BAND)).sum(axis=1)
        le = (ok[:, None] & (diff < -BAND)).sum(axis=1)
        band = (ok[:, None] & (np.abs(diff) <= BAND)).sum(axis=1)
    return ge.astype(np.int64), le.astype(np.int64), band.astype(np.int64)


def band_share(N: int, K: int, kind: str):
    """(pairs inside the band, scored pairs) of a fixture."""
    band = counts_bracket(N, K, kind)[2]
    return int(band.sum()), int((~np.isnan(observed_oracle(N, K, kind))).sum()) * P
