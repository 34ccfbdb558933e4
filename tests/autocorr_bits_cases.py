"""The recorded bits of every spatial-autocorrelation entry (TEST INFRASTRUCTURE ONLY): what tests/test_hip_autocorr_bits.py
recomputes and tests/golden/make_autocorr_bits_golden.py stores in tests/golden/extra_autocorr_bits.npz.

The gene pass (gene_morans_i_sparse, gene_spatial_stats_sparse, the observed statistic of the permutation entries) and the
column pass (morans_i, spatial_stats, residual_morans_i) each exist once in the library, instantiated narrow (Moran's I
alone) and wide (with Geary's C and the moments).  The tests that compare one entry with another therefore compare a kernel
with itself; this fixture pins the numbers from outside.  Every fp64 output is kept as its int64 view, so NaNs compare too.

Inputs are regenerated, never stored: ``gene_rank_cases.counts`` / ``graph``, the fp32 square root of the counts as
non-integer data (IEEE square root is correctly rounded: the same on every machine), and ``residual_cases.make_case``.

  gene/...      (N, K) in GENE_SHAPES x variant x data: N = 257 is one spot past a 256-entry sweep, N = 1037 rows of five
  column/...    the last L of the 74 columns [counts.T, root-counts.T] (so L = 1 is a scored gene, L = 70 holds every row
                kind), fp32 and fp64, K = 6: L = 70 is a second column tile, N = 7 / 257 / 1037 one, two and five row chunks
  perm/...      the four permutation functions, line_mode 1 and 2, perm_batch 0 and 2, P = 5 with the identity third:
                sparse rows on the integer counts with holes (ties are exact), dense rows on the root-counts
  residual/...  the smallest case of residual_cases.TABLE, dense and sparse counts, Poisson/Pearson and NB/deviance: a slab
                of 64 columns of which one is scored, so the row stride differs from the column count
  plan/...      the plan queries' returned values (host only), keys sorted"""
from __future__ import annotations

import os

import numpy as np

import gene_rank_cases as G
import residual_cases as R

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extra_autocorr_bits.npz")

GENE_SHAPES = ((7, 6), (257, 1), (1037, 6), (1037, 32))
DATA = ("counts", "root")
COLUMN_LS = (1, 5, 70)
COLUMN_NS = (7, 257, 1037)
COLUMN_K = 6
PERM_SHAPES = ((257, 6), (1037, 32))
PERM_P = 5
LINE_MODES = (1, 2)
PERM_BATCHES = (0, 2)
STAT_FIELDS = ("I", "C", "mean", "var", "kurtosis")
PERM_FIELDS = ("n_ge", "n_le", "sim_mean", "sim_m2", "sims")
RESIDUAL_CASE = R.TABLE[0][0]
RESIDUAL_COMBOS = (("poisson", "pearson"), ("nb", "deviance"))


def values(N: int, variant: str, data: str) -> np.ndarray:
    """(D, N) float32: the counts, or their fp32 square root."""
    Y = G.counts(N, variant)
    return Y if data == "counts" else np.sqrt(Y, dtype=np.float32)


def columns(N: int, L: int) -> np.ndarray:
    """(N, L) float64 holding fp32 values."""
    both = np.concatenate([values(N, "full", "counts").T, values(N, "full", "root").T], axis=1)
    return np.ascontiguousarray(both[:, -L:], dtype=np.float64)


def perms(N: int) -> np.ndarray:
    """(PERM_P, N) int32, the identity third."""
    rng = np.random.default_rng(11 + N)
    out = np.stack([rng.permutation(N) for _ in range(PERM_P)]).astype(np.int32)
    out[2] = np.arange(N)
    return out


def bits(t) -> np.ndarray:
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return a.view(np.int64).copy() if a.dtype == np.float64 else a.copy()


def _plan(d: dict) -> np.ndarray:
    return np.array([int(d[k]) for k in sorted(d)], dtype=np.int64)


def plans() -> dict:
    """Every plan query of the family (no device needed)."""
    from gpzoo_amd import ops
    out = {}
    for N, K in GENE_SHAPES:
        for variant in G.VARIANTS:
            nnz = int(np.count_nonzero(G.counts(N, variant)))
            out[f"plan/gene_rank/{N}_{K}_{variant}"] = _plan(ops.gene_rank_plan(N, G.D, nnz, K=K))
            out[f"plan/gene_stats/{N}_{K}_{variant}"] = _plan(ops.spatial_stats_plan(N, K, D=G.D, nnz=nnz))
    for N in COLUMN_NS:
        for L in COLUMN_LS:
            out[f"plan/column_stats/{N}_{L}"] = _plan(ops.spatial_stats_plan(N, COLUMN_K, L=L))
    for N, K in PERM_SHAPES:
        for nnz in (None, int(np.count_nonzero(G.counts(N, "holes")))):
            rows = "dense" if nnz is None else "sparse"
            for lm in (0,) + LINE_MODES:
                for pb in PERM_BATCHES:
                    key = f"{rows}_{N}_{K}_lm{lm}_pb{pb}"
                    out[f"plan/morans_perm/{key}"] = _plan(ops.morans_perm_plan(N, G.D, K, PERM_P, nnz, pb, lm))
                    for stat in ("moran", "geary"):
                        out[f"plan/autocorr_perm/{stat}_{key}"] = _plan(ops.autocorr_perm_plan(N, G.D, K, PERM_P, nnz, stat, pb, lm))
    c = R.make_case(RESIDUAL_CASE)
    for nnz in (0, int(np.count_nonzero(c["y"]))):
        out[f"plan/residual/nnz{nnz}"] = _plan(ops.residual_autocorr_plan(c["B"], c["D"], c["Lt"], nnz))
    return out


def gene_entries() -> dict:
    import torch
    from gpzoo_amd import ops
    from gpzoo_amd.likelihoods import SparseCounts
    out = {}
    for N, K in GENE_SHAPES:
        nbr = torch.tensor(G.graph(N, K)).cuda()
        for variant in G.VARIANTS:
            for data in DATA:
                v = SparseCounts(torch.tensor(values(N, variant, data))).cuda()
                key = f"gene/{N}_{K}_{variant}_{data}"
                out[f"{key}/morans_i"] = bits(ops.gene_morans_i_sparse(v, nbr))
                s = ops.gene_spatial_stats_sparse(v, nbr)
                for f in STAT_FIELDS:
                    out[f"{key}/stats_{f}"] = bits(getattr(s, f))
    return out


def column_entries() -> dict:
    import torch
    from gpzoo_amd import ops
    out = {}
    for N in COLUMN_NS:
        nbr = torch.tensor(G.graph(N, COLUMN_K)).cuda()
        for L in COLUMN_LS:
            for dtype in (torch.float32, torch.float64):
                V = torch.tensor(columns(N, L), dtype=dtype).cuda()
                key = f"column/{N}_{L}_{'f32' if dtype == torch.float32 else 'f64'}"
                out[f"{key}/morans_i"] = bits(ops.morans_i(V, nbr))
                s = ops.spatial_stats(V, nbr)
                for f in STAT_FIELDS:
                    out[f"{key}/stats_{f}"] = bits(getattr(s, f))
    return out


def perm_entries() -> dict:
    import torch
    from gpzoo_amd import ops
    from gpzoo_amd.likelihoods import SparseCounts
    out = {}
    for N, K in PERM_SHAPES:
        nbr, pi = torch.tensor(G.graph(N, K)).cuda(), torch.tensor(perms(N)).cuda()
        sparse = SparseCounts(torch.tensor(values(N, "holes", "counts"))).cuda()
        dense = torch.tensor(values(N, "full", "root")).cuda()
        for lm in LINE_MODES:
            for pb in PERM_BATCHES:
                kw = dict(return_sims=True, perm_batch=pb, line_mode=lm)
                runs = {"sparse/morans": ops.gene_morans_perm_sparse(sparse, nbr, pi, **kw),
                        "dense/morans": ops.morans_perm_rows(dense, nbr, pi, **kw)}
                for stat in ("moran", "geary"):
                    runs[f"sparse/autocorr_{stat}"] = ops.gene_autocorr_perm_sparse(sparse, nbr, pi, stat=stat, **kw)
                    runs[f"dense/autocorr_{stat}"] = ops.autocorr_perm_rows(dense, nbr, pi, stat=stat, **kw)
                for name, r in runs.items():
                    key = f"perm/{N}_{K}_lm{lm}_pb{pb}/{name}"
                    out[f"{key}/value"] = bits(r.I if hasattr(r, "I") else r.value)
                    for f in PERM_FIELDS:
                        out[f"{key}/{f}"] = bits(getattr(r, f))
    return out


def residual_entries() -> dict:
    import torch
    from gpzoo_amd import ops
    from gpzoo_amd.likelihoods import SparseCounts
    c = R.make_case(RESIDUAL_CASE)
    d = {k: torch.tensor(np.asarray(c[k]), dtype=torch.float32).cuda() for k in ("mean", "scale", "W", "V", "y", "theta")}
    nbr = torch.tensor(R.case_table(c)).cuda()
    out = {}
    for rows, y in (("dense", d["y"]), ("sparse", SparseCounts(d["y"]))):
        for family, kind in RESIDUAL_COMBOS:
            r = ops.residual_morans_i(d["mean"], d["scale"], d["W"], d["V"], y, nbr,
                                      theta_pos=d["theta"] if family == "nb" else None, kind=kind)
            for f in ("I", "residual_mean", "residual_var"):
                out[f"residual/{rows}_{family}_{kind}/{f}"] = bits(r[f])
    return out


GROUPS = {"gene": gene_entries, "column": column_entries, "perm": perm_entries, "residual": residual_entries}
