#!/usr/bin/env python3
"""Time the entries that give Geary's C and the moments beside Moran's I (gpz_gene_spatial_stats_sparse,
gpz_gene_autocorr_perm_sparse with stat = 1) against the Moran-only entries they extend, on one GPU, in one process, at the
Slide-seq shape (D = 17702 genes, N = 39694 spots, K = 6 neighbours, P = 100 permutations) at 1 / 5 / 20 % density:
  moran_i       ``ops.gene_morans_i_sparse``                        stats        ``ops.gene_spatial_stats_sparse`` (I, C, mean, var, b2)
  moran_perm    ``ops.gene_morans_perm_sparse``                     geary_perm   ``ops.gene_autocorr_perm_sparse(stat="geary")``
  moran_perm_stat0   ``ops.gene_autocorr_perm_sparse(stat="moran")``: the Moran-only entry's kernels through the new entry
The arms alternate round by round after a warm-up; the median (and minimum) of --reps rounds (>= 30) is reported, with the
ratio of each new entry to the Moran-only one and whether the shared outputs have the same bits.  One JSON line per density.

    python tools/geary_step.py [--reps 30] [--density 0.01 0.05 0.2] [--perms 100] [--json FILE]"""
import argparse
import gc
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402
from moran_perm_step import measure, sparse_counts  # noqa: E402


def run(D, N, K, P, density, reps, dev):
    gc.collect()
    torch.cuda.empty_cache()
    c = sparse_counts(D, N, density, dev)
    X = torch.rand(N, 2, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(dev)
    nbr = ops.spatial_knn(X, K)
    g = torch.Generator(device=dev).manual_seed(3)
    perms = torch.stack([torch.randperm(N, generator=g, device=dev) for _ in range(P)]).to(torch.int32)
    arms = {"moran_i": lambda: ops.gene_morans_i_sparse(c, nbr),
            "stats": lambda: ops.gene_spatial_stats_sparse(c, nbr),
            "moran_perm": lambda: ops.gene_morans_perm_sparse(c, nbr, perms),
            "moran_perm_stat0": lambda: ops.gene_autocorr_perm_sparse(c, nbr, perms, stat="moran"),
            "geary_perm": lambda: ops.gene_autocorr_perm_sparse(c, nbr, perms, stat="geary")}
    ms, out = measure(arms, reps)
    res = dict(D=D, N=N, K=K, P=P, density=density, nnz=c.nnz, reps=reps)
    for k in arms:
        res[k + "_ms"] = round(ms[k][0], 3)
        res[k + "_min_ms"] = round(ms[k][1], 3)
    same = lambda s, t: bool(torch.equal(torch.nan_to_num(s, nan=-7.0), torch.nan_to_num(t, nan=-7.0)))  # noqa: E731
    a, b = out["moran_perm"], out["moran_perm_stat0"]
    res.update(stats_over_moran_i=round(ms["stats"][0] / ms["moran_i"][0], 3),
               geary_perm_over_moran_perm=round(ms["geary_perm"][0] / ms["moran_perm"][0], 3),
               stat0_over_moran_perm=round(ms["moran_perm_stat0"][0] / ms["moran_perm"][0], 3),
               stats_I_same_bits=same(out["stats"].I, out["moran_i"]),
               geary_perm_C_same_bits=same(out["geary_perm"].value, out["stats"].C),
               stat0_same_bits=same(a.I, b.value) and same(a.sim_mean, b.sim_mean) and same(a.sim_m2, b.sim_m2)
               and bool(torch.equal(a.n_ge, b.n_ge) and torch.equal(a.n_le, b.n_le)))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--density", type=float, nargs="+", default=[0.01, 0.05, 0.2])
    ap.add_argument("--genes", type=int, default=17702)
    ap.add_argument("--spots", type=int, default=39694)
    ap.add_argument("--neighbours", type=int, default=6)
    ap.add_argument("--perms", type=int, default=100)
    ap.add_argument("--json", default=None, help="append the result lines to this file too")
    a = ap.parse_args()
    dev = torch.device("cuda")
    for density in a.density:
        res = run(a.genes, a.spots, a.neighbours, a.perms, density, max(a.reps, 30), dev)
        if a.json:
            with open(a.json, "a") as f:
                f.write(json.dumps(res) + "\n")
        ops.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
