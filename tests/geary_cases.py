"""Seeded cases, fp64 / integer oracles and the recorded tolerances for Geary's C, the kurtosis and the randomisation moments
(gpzoo_amd/csrc/spatial_stats.hip, moran_expr.h; ``utilities.gene_autocorr(mode="geary", assumption="randomisation")``).
TEST INFRASTRUCTURE ONLY; numpy, everything runs on the CPU.

The data are those of tests/gene_rank_cases.py and tests/moran_perm_cases.py (D = 37 genes with their row kinds, N in NS, the
tables of GRAPHS, the fixtures "counts" / "log", P = 19 permutations per N), plus one tiny enumeration fixture: N = 7, three
tables, three genes and all 7! = 5040 relabellings, over which the mean and the variance of I and C are the analytic
randomisation moments exactly.

Tolerances, and where each comes from:

  GEARY_ATOL_ROWS    = MORAN_ATOL (1e-10), for the dense-columns entry: its sums are centred and non-negative, as Moran's there.
  GEARY_ATOL_SPARSE  = 4 x EMULATION_WORST, capped at 1e-9.  EMULATION_WORST is the largest |geary_expanded - geary_oracle| over
                       every fixture here (emulation_worst(); N in NS, K in KS, "counts" and "log", "full" and "holes"), recorded
                       below and checked by tests/test_geary_cases.py: the plain expansion G = K Q + Q_in - 2 C_s over
                       K (Q - N xbar^2) in sequential fp64 sums.  The margin of 4 is there because the device adds 256 strided
                       partial sums and a binary tree, not a sequence.  The worst case is the every-spot "log" gene at N = 4099,
                       whose mean^2 / variance is large: as with Moran's I in this form, digits are lost in proportion to
                       mean^2 / variance, in G as in the denominator.  On every integer fixture the error is <= 1.1e-13.
  KURTOSIS_RTOL      = 1e-11: fp64 epsilon x 4099 sequential terms x ~20, the rule of DEVIANCE_RTOL; the two-sweep centred form
                       has no cancellation.
  moments            against moments() at the device's own b2: 1e-12 relative (the rule of gene_rank_cases.moments_bound);
                       1e-15 absolute over the complete graph (K = N - 1), where C = 1 whatever the values and its variance is 0.
  ENUM_RTOL          = 1e-9 for the device's mean_sim / var_sim over all 5040 relabellings against the analytic moments: the
                       N = 7 errors of the statistic are ~3e-12, and the gap to the normality variance is >= 10 %.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import gene_rank_cases as G
import moran_perm_cases as M

GEARY_ATOL_ROWS = G.MORAN_ATOL
EMULATION_WORST = 1.2e-10          # emulation_worst() on this code; tests/test_geary_cases.py keeps it honest
GEARY_ATOL_SPARSE = min(1e-9, 4.0 * EMULATION_WORST)
KURTOSIS_RTOL = 1e-11
ENUM_RTOL = 1e-9
BAND = 2.0 * GEARY_ATOL_SPARSE     # |C_pi - C| of two values each within GEARY_ATOL_SPARSE of its oracle
FIXTURES = [(kind, variant) for kind in ("counts", "log") for variant in G.VARIANTS]


@functools.lru_cache(maxsize=None)
def values(N: int, kind: str, variant: str) -> np.ndarray:
    """(D, N) float32 values of a fixture."""
    out = G.counts(N, variant) if kind == "counts" else G.log_values(N, variant)[1]
    out.setflags(write=False)
    return out


# ---- oracles ---------------------------------------------------------------------------------------------------------

def geary_oracle(dense, nbr):
    """(D,) Geary's C of every gene of dense (D, N), zeros included: direct centred sums, C = (N - 1) sum_i sum_{j in nbr(i)}
    (z_i - z_j)^2 / (2 N K sum z^2), sums of non-negative fp64 terms.  NaN for a constant gene."""
    X = np.asarray(dense, dtype=np.float64)
    N, K = nbr.shape
    Z = X - X.mean(axis=1, keepdims=True)
    Gs = ((Z[:, :, None] - Z[:, nbr]) ** 2).sum(axis=(1, 2))
    den = (Z * Z).sum(axis=1)
    const = X.min(axis=1) == X.max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(const, np.nan, (N - 1) * Gs / (2 * N * K * np.where(const, 1, den)))
    return out


def kurtosis_oracle(dense):
    """dict(mean, var, kurtosis), (D,) fp64 each: m_k = sum (x - mean)^k / N in extended precision, b2 = m4 / m2^2, NaN for a
    constant gene."""
    X = np.asarray(dense, dtype=np.longdouble)
    mean = X.mean(axis=1)
    Z = X - mean[:, None]
    m2, m4 = (Z ** 2).mean(axis=1), (Z ** 4).mean(axis=1)
    const = X.min(axis=1) == X.max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        b2 = np.where(const, np.nan, m4 / np.where(const, 1, m2 * m2))
    return dict(mean=mean.astype(np.float64), var=m2.astype(np.float64), kurtosis=b2.astype(np.float64))


@functools.lru_cache(maxsize=None)
def _graph_sums(key):
    nbr = np.frombuffer(key[0], dtype=np.int64).reshape(key[1])
    N = nbr.shape[0]
    W = np.zeros((N, N))
    W[np.arange(N)[:, None], nbr] = 1.0
    return float(W.sum()), float(0.5 * ((W + W.T) ** 2).sum()), float(((W.sum(axis=1) + W.sum(axis=0)) ** 2).sum())


def moments(nbr, b2):
    """The moments of I and C from the dense binary W as PySAL forms S0, S1, S2: dict(EI, EC, VI_norm, VC_norm) and, per entry
    of b2 (any shape), VI_rand, VC_rand (Cliff & Ord; PySAL's VI_rand, VC_rand)."""
    nbr = np.ascontiguousarray(nbr, dtype=np.int64)
    S0, S1, S2 = _graph_sums((nbr.tobytes(), nbr.shape))
    n = float(nbr.shape[0])
    b2 = np.asarray(b2, dtype=np.float64)
    EI = -1.0 / (n - 1)
    VI_norm = (n * n * S1 - n * S2 + 3 * S0 * S0) / ((n * n - 1) * S0 * S0) - EI * EI
    VI_rand = ((n * ((n * n - 3 * n + 3) * S1 - n * S2 + 3 * S0 * S0) - b2 * ((n * n - n) * S1 - 2 * n * S2 + 6 * S0 * S0))
               / ((n - 1) * (n - 2) * (n - 3) * S0 * S0) - EI * EI)
    VC_norm = ((2 * S1 + S2) * (n - 1) - 4 * S0 * S0) / (2 * (n + 1) * S0 * S0)
    VC_rand = (((n - 1) * S1 * (n * n - 3 * n + 3 - (n - 1) * b2) - 0.25 * (n - 1) * S2 * (n * n + 3 * n - 6 - (n * n - n + 2) * b2)
                + S0 * S0 * (n * n - 3 - (n - 1) ** 2 * b2)) / (n * (n - 2) * (n - 3) * S0 * S0))
    return dict(EI=EI, EC=1.0, VI_norm=VI_norm, VC_norm=VC_norm, VI_rand=VI_rand, VC_rand=VC_rand)


def moments_bound(N, K, V):
    """|variance - oracle| allowed: gene_rank_cases.moments_bound's rule, per entry of V."""
    return np.full(np.shape(V), 1e-15) if K == N - 1 else 1e-12 * np.abs(V)


def expansion_sums(x, nz, row, nbr, indeg):
    """(S, Q, C_s, Q_in) of one gene over its stored spots nz, as sequential sums (np.cumsum adds in order)."""
    lag = np.cumsum(row[nbr[nz]], axis=1)[:, -1]
    return tuple(np.cumsum(v)[-1] for v in (x, x * x, x * lag, indeg[nz] * (x * x)))


def geary_expanded(dense, nbr):
    """The expression the sparse kernel evaluates, in numpy with sequential fp64 sums over the stored entries, every product
    and sum rounded on its own: G = K Q + Q_in - 2 C_s, C = (N - 1) G / (2 N K (Q - N xbar^2))."""
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
        S, Q, Cs, Qin = expansion_sums(x, nz, X[d], nbr, indeg)
        xbar = S / N
        den = K * (Q - N * (xbar * xbar))
        if den > 0:
            out[d] = ((N - 1.0) * (K * Q + Qin - 2.0 * Cs)) / (2.0 * N * den)
    return out


def emulation_error(N, K, kind, variant):
    """max |geary_expanded - geary_oracle| over the scored genes of a fixture (the NaN patterns must agree)."""
    X, nbr = values(N, kind, variant), G.graph(N, K)
    a, b = geary_expanded(X, nbr), geary_oracle(X, nbr)
    assert (np.isnan(a) == np.isnan(b)).all()
    return float(np.nanmax(np.abs(a - b)))


def emulation_worst():
    return max(emulation_error(N, K, kind, variant) for N, K in G.GRAPHS for kind, variant in FIXTURES)


# ---- the permutation null -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sims_oracle(N: int, K: int, kind: str) -> np.ndarray:
    """(D, P) fp64: geary_oracle on the permuted dense array of moran_perm_cases' fixture, per permutation."""
    X, nbr = M.dense(N, kind), G.graph(N, K)
    out = np.stack([geary_oracle(X[:, pi], nbr) for pi in M.perms(N)], axis=1)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def observed_oracle(N: int, K: int, kind: str) -> np.ndarray:
    out = geary_oracle(M.dense(N, kind), G.graph(N, K))
    out.setflags(write=False)
    return out


def _order_statistic(X, nbr, indeg):
    """Per gene, Q_in - 2 C_s in Python integers (X int64 (D, N))."""
    Cs = (X * X[:, nbr].sum(axis=2)).sum(axis=1)
    Qin = (X * X * indeg).sum(axis=1)
    return [int(q) - 2 * int(c) for q, c in zip(Qin, Cs)]


@functools.lru_cache(maxsize=None)
def counts_oracle_exact(N: int, K: int):
    """(n_ge, n_le), int64 (D,): the permutations with C_pi >= C and C_pi <= C for the integer "counts" fixture, decided on
    Q_in - 2 C_s in integers (K Q and the denominator do not depend on pi).  A gene without C counts nothing."""
    Y = M.dense(N, "counts")
    X = Y.astype(np.int64)
    assert (X == Y).all()
    nbr = G.graph(N, K)
    indeg = np.bincount(nbr.reshape(-1), minlength=N).astype(np.int64)
    t0 = _order_statistic(X, nbr, indeg)
    scored = [N * int(q) - int(s) ** 2 > 0 for q, s in zip((X * X).sum(axis=1), X.sum(axis=1))]
    n_ge, n_le = np.zeros(G.D, dtype=np.int64), np.zeros(G.D, dtype=np.int64)
    for pi in M.perms(N):
        t = _order_statistic(X[:, pi], nbr, indeg)
        for d in range(G.D):
            if scored[d]:
                n_ge[d] += t[d] >= t0[d]
                n_le[d] += t[d] <= t0[d]
    return n_ge, n_le


def counts_bracket(N: int, K: int, kind: str):
    """moran_perm_cases.counts_bracket's construction for C with BAND = 2 GEARY_ATOL_SPARSE: (ge, le, band), int64 (D,)."""
    C, sims = observed_oracle(N, K, kind), sims_oracle(N, K, kind)
    ok = ~np.isnan(C)
    assert (np.isnan(sims) == ~ok[:, None]).all()
    with np.errstate(invalid="ignore"):
        diff = sims - C[:, None]
        ge = (ok[:, None] & (diff > BAND)).sum(axis=1)
        le = (ok[:, None] & (diff < -BAND)).sum(axis=1)
        band = (ok[:, None] & (np.abs(diff) <= BAND)).sum(axis=1)
    return ge.astype(np.int64), le.astype(np.int64), band.astype(np.int64)


def band_share(N: int, K: int, kind: str):
    """(pairs inside the band, scored pairs) of a fixture."""
    band = counts_bracket(N, K, kind)[2]
    return int(band.sum()), int((~np.isnan(observed_oracle(N, K, kind))).sum()) * M.P


# ---- full enumeration at N = 7 --------------------------------------------------------------------------------------------

ENUM_N = 7
ENUM_TABLES = {
    "ring13": np.array([[(i + 1) % 7, (i + 3) % 7] for i in range(7)], dtype=np.int64),
    "ring112": np.array([[(i + 1) % 7, (i - 1) % 7, (i + 2) % 7] for i in range(7)], dtype=np.int64),
    "irregular": np.array([[1, 2], [0, 2], [0, 1], [0, 1], [0, 3], [4, 0], [5, 1]], dtype=np.int64),      # in-degrees 5 4 2 1 1 1 0
}
ENUM_GENES = np.stack([np.array([0, 3, 0, 0, 1, 0, 7], dtype=np.float64), np.log1p(np.array([0, 3, 2, 0, 1, 5, 7], dtype=np.float64)),
                       np.array([1, 1, 2, 1, 9, 1, 3], dtype=np.float64)]).astype(np.float32)            # the last: stored at every spot


@functools.lru_cache(maxsize=None)
def enum_perms() -> np.ndarray:
    """All 5040 permutations of 0 .. 6 as a (5040, 7) int32 table, the identity first."""
    out = np.array(list(itertools.permutations(range(ENUM_N))), dtype=np.int32)
    out.setflags(write=False)
    return out


def enum_statistics(x, nbr):
    """(I, C), (5040,) each: both statistics of the gene x under every relabelling x[pi], direct centred fp64 sums."""
    X = np.asarray(x, dtype=np.float64)[enum_perms()]
    N, K = nbr.shape
    Z = X - X.mean(axis=1, keepdims=True)
    den = (Z * Z).sum(axis=1)
    I = (Z * Z[:, nbr].sum(axis=2)).sum(axis=1) / (K * den)
    C = (N - 1) * ((Z[:, :, None] - Z[:, nbr]) ** 2).sum(axis=(1, 2)) / (2 * N * K * den)
    return I, C
