#!/usr/bin/env python3
"""Time the two per-gene scores of a ``SparseCounts`` (gpz_gene_deviance_sparse, gpz_gene_morans_i_sparse) on one GPU, in
one process, at the Slide-seq shape (D = 17702 genes, N = 39694 spots, K = 6 neighbours) at 1 / 5 / 20 % density, against
what a user composes without them:
  moran_dense      ``ops.morans_i`` on the densified (N, D) array (densify_transpose, the ``to_dense().T.contiguous()`` it
                   needs first, is timed on its own)
  deviance_torch   the Poisson deviance as torch ops over the stored entries (gather, log, ``_segment_sums``)
The arms alternate round by round after a warm-up; the median (and minimum) of --reps rounds (>= 30) is reported, with the
largest differences between the arms' results.  One JSON line per density.

    python tools/gene_rank_step.py [--reps 30] [--density 0.01 0.05 0.2] [--genes 17702 --spots 39694 --neighbours 6]"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd.likelihoods import SparseCounts, _segment_sums  # noqa: E402
from gpzoo_amd.utilities import _spot_totals_tensor  # noqa: E402


def sparse_counts(D, N, density, dev):
    """Counts of 1 .. 8 at ``density`` of the positions, drawn on the device."""
    g = torch.Generator(device=dev).manual_seed(1)
    counts = torch.rand(D, N, generator=g, device=dev)
    counts = (counts < density) * (1.0 + torch.floor(8.0 * torch.rand(D, N, generator=g, device=dev)))
    return SparseCounts(counts)


def deviance_torch(c, size):
    """The Poisson gene deviance composed from torch ops: O(nnz) temporaries in fp64."""
    perm = c.row_perm.long()
    y = c.col_val[perm].to(torch.float64)
    sat = _segment_sums(y * torch.log(y / size[c.row_spot.long()]), c.row_ptr)
    s = _segment_sums(y, c.row_ptr)
    null = torch.where(s > 0, s * torch.log(s / size.sum()), torch.zeros_like(s))
    return 2.0 * (sat - null)


def measure(arms, reps, warmup=3):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out, ts = {}, {k: [] for k in arms}
    for k, fn in arms.items():
        for _ in range(warmup):
            out[k] = fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in arms.items():
            ev0.record(); out[k] = fn(); ev1.record(); torch.cuda.synchronize()
            ts[k].append(ev0.elapsed_time(ev1))
    return {k: (statistics.median(v), min(v)) for k, v in ts.items()}, out


def run(D, N, K, density, reps, dev):
    gc.collect()
    torch.cuda.empty_cache()
    c = sparse_counts(D, N, density, dev)
    size = _spot_totals_tensor(c).clamp_min(1.0)
    X = torch.rand(N, 2, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(dev)
    nbr = ops.spatial_knn(X, K)
    dense_t = c.to_dense().T.contiguous()
    arms = {"moran_sparse": lambda: ops.gene_morans_i_sparse(c, nbr),
            "moran_dense": lambda: ops.morans_i(dense_t, nbr),
            "densify_transpose": lambda: c.to_dense().T.contiguous(),
            "deviance_sparse": lambda: ops.gene_deviance_sparse(c, size, 0)[2],
            "deviance_binomial_sparse": lambda: ops.gene_deviance_sparse(c, size, 1)[2],
            "deviance_torch": lambda: deviance_torch(c, size)}
    ms, out = measure(arms, reps)
    res = dict(D=D, N=N, K=K, density=density, nnz=c.nnz, reps=reps)
    for k in arms:
        res[k + "_ms"] = round(ms[k][0], 4)
        res[k + "_min_ms"] = round(ms[k][1], 4)
    a, b = out["moran_sparse"], out["moran_dense"]
    ok = ~(torch.isnan(a) | torch.isnan(b))
    res.update(moran_sparse_over_dense=round(ms["moran_sparse"][0] / ms["moran_dense"][0], 3),
               moran_sparse_over_dense_with_densify=round(ms["moran_sparse"][0] / (ms["moran_dense"][0] + ms["densify_transpose"][0]), 3),
               deviance_sparse_over_torch=round(ms["deviance_sparse"][0] / ms["deviance_torch"][0], 3),
               moran_scratch_mib=round(ops.gene_rank_plan(N, D, c.nnz, K=K)["partials_bytes"] / 2 ** 20, 1),
               dense_mib=round(4 * D * N / 2 ** 20, 1),
               moran_max_abs_diff=float((a - b)[ok].abs().max()), moran_nan_agree=bool(torch.equal(torch.isnan(a), torch.isnan(b))),
               deviance_max_rel_diff=float(((out["deviance_sparse"] - out["deviance_torch"]).abs()
                                            / out["deviance_torch"].abs().clamp_min(1e-300)).max()))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--density", type=float, nargs="+", default=[0.01, 0.05, 0.2])
    ap.add_argument("--genes", type=int, default=17702)
    ap.add_argument("--spots", type=int, default=39694)
    ap.add_argument("--neighbours", type=int, default=6)
    a = ap.parse_args()
    dev = torch.device("cuda")
    for density in a.density:
        run(a.genes, a.spots, a.neighbours, density, max(a.reps, 30), dev)
        ops.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
