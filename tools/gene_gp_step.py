#!/usr/bin/env python3
"""Time the steps of gene_spatial_gp on one GPU and print one JSON line.

    python tools/gene_gp_step.py [--densities 0.01,0.05,0.2] [--reps 30] [--genes 17702] [--spots 39694] [--inducing 256]

Shape: the Slide-seq one, D = 17 702 genes, N = 39 694 spots, d = 2, M = 256 inducing points (k-means), 8 length scales
(the default grid), RBF; stored entries uniform at the given densities, values log1p(1 .. 8).

Per density, three arms alternate in one process after two warm-up rounds, each call between two device events, `reps`
rounds, median / min / max in ms:
  project_ms      ops.gene_kernel_project_sparse: K_zx Y^T for all length scales, K_zx generated and never stored
  yardstick_ms    what the library composes without it, per length scale: ops.kfill of the fp64 K_xz (N x M), then
                  ops.counts_matmul of the stored values with it in column blocks of 128
  yardstick2_ms   the same composition again: the spread between the two is the noise of the comparison
`max_rel_diff`: the largest difference between the two results over the largest entry.  `project_partials_mb`: the plan's
scratch; `yardstick_kxz_mb`: the N x M x 8 bytes per length scale the composition allocates.
At the first density also: `gram_ms` (ops.kernel_gram, K_zx K_xz and K_zx 1), `algebra_ms` (Cholesky, solves, eigh, and the
rotation matmul; host clock, eigh may run on the host), `profile_ms` (ops.gene_gp_profile), `end_to_end_ms`
(gene_spatial_gp with Z given; host clock) and `end_to_end_peak_mb` (torch's peak allocation over what was held before)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd import utilities as ut  # noqa: E402
from gpzoo_amd.likelihoods import SparseCounts, SparseExpression, _gene_moments  # noqa: E402


def stats(ms):
    return {"median": round(float(np.median(ms)), 3), "min": round(float(np.min(ms)), 3), "max": round(float(np.max(ms)), 3)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--densities", default="0.01,0.05,0.2")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--genes", type=int, default=17702)
    ap.add_argument("--spots", type=int, default=39694)
    ap.add_argument("--inducing", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda")
    D, N, M = args.genes, args.spots, args.inducing
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand((N, 2), generator=gen, device=dev, dtype=torch.float64)
    Z = ut.kmeans_inducing_points(X, M, random_state=0).contiguous()
    ell = ut._default_lengthscales(X, M)
    nl = int(ell.numel())
    spec = ops.KernelSpec(ops.GENE_GP_KINDS["rbf"], torch.ones(nl, dtype=torch.float64, device=dev), ell, True)
    out = {"tool": "gene_gp_step", "D": D, "N": N, "M": M, "n_ell": nl, "kernel": "rbf", "reps": args.reps, "densities": {}}
    for i, density in enumerate(float(v) for v in args.densities.split(",")):
        y = torch.zeros((D, N), device=dev)
        for lo in range(0, D, 2048):                    # a slab at a time: the mask and the draws are temporaries
            hi = min(lo + 2048, D)
            mask = torch.rand((hi - lo, N), generator=gen, device=dev) < density
            y[lo:hi] = torch.log1p(torch.randint(1, 9, (hi - lo, N), generator=gen, device=dev).float()) * mask
        values = SparseCounts(y)
        del y, mask
        zero = torch.zeros(D, dtype=torch.float64, device=dev)
        expr = SparseExpression(values, _gene_moments(SparseExpression(values, zero))[0] / N)
        plan = ops.gene_kernel_project_plan(N, D, values.nnz, M, nl)
        r = {"nnz": values.nnz, "gene_chunk": plan["gene_chunk"], "generate": plan["generate"], "project_partials_mb": round(plan["partials_bytes"] / 2 ** 20, 1),
             "yardstick_kxz_mb": round(N * M * 8 / 2 ** 20, 1)}

        def project():
            return ops.gene_kernel_project_sparse(values, X, Z, ell, "rbf")

        def yardstick():
            res = torch.empty((nl, D, M), dtype=torch.float64, device=dev)
            for l in range(nl):
                one = ops.KernelSpec(spec.kind, spec.sigma[l:l + 1], ell[l:l + 1], False)
                Kxz = ops.kfill(one, X, Z)                                   # (N, M) fp64
                for m0 in range(0, M, 128):
                    res[l, :, m0:m0 + 128] = ops.counts_matmul(values, Kxz[:, m0:m0 + 128].contiguous(), transpose=True)
            return res

        arms = {"project_ms": project, "yardstick_ms": yardstick, "yardstick2_ms": yardstick}
        for _ in range(2):
            got = {k: fn() for k, fn in arms.items()}
        r["max_rel_diff"] = float((got["project_ms"] - got["yardstick_ms"]).abs().max() / got["yardstick_ms"].abs().max())
        del got
        ms = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, fn in arms.items():
                t, res = event_ms(fn)
                del res
                ms[k].append(t)
        r.update({k: stats(v) for k, v in ms.items()})
        if i == 0:
            ones = torch.ones((nl, N), dtype=torch.float64, device=dev)
            r["gram_ms"] = stats([event_ms(lambda: ops.kernel_gram(spec, Z, X, ones, 0.0))[0] for _ in range(args.reps + 2)][2:])
            G, b = ops.kernel_gram(spec, Z, X, ones, 0.0)
            P = project()

            def algebra():
                Kzz = ops.kfill(spec, Z, Z) + 1e-6 * torch.eye(M, dtype=torch.float64, device=dev)
                Lz = torch.tril(ops.cholesky(Kzz))
                B = ops.solve_triangular_lower(Lz, ops.solve_triangular_lower(Lz, G).transpose(-1, -2).contiguous())
                lam, U = ut._eigh(0.5 * (B + B.transpose(-1, -2)))
                W = torch.linalg.solve_triangular(Lz.transpose(-1, -2), U, upper=True)
                return lam.clamp_min(0.0).contiguous(), torch.matmul(P - expr.offset[None, :, None] * b, W)

            for _ in range(2):
                lam, p = algebra()
            r["algebra_ms"] = stats([host_ms(algebra)[0] for _ in range(5)])
            del P
            sz, szz = _gene_moments(expr)
            yty = (szz - 2.0 * expr.offset * sz + N * expr.offset * expr.offset).contiguous()
            r["profile_ms"] = stats([event_ms(lambda: ops.gene_gp_profile(p, lam, yty, N))[0] for _ in range(args.reps + 2)][2:])
            del p

            def whole():
                return ut.gene_spatial_gp(expr, X, inducing=Z, lengthscales=ell)

            whole()
            r["end_to_end_ms"] = stats([host_ms(whole)[0] for _ in range(3)])
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            res = whole()
            torch.cuda.synchronize()
            r["end_to_end_peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            r["status_counts"] = [int((res.status == k).sum()) for k in range(4)]
            del res
        out["densities"][str(density)] = r
        print(json.dumps({str(density): r}), file=sys.stderr, flush=True)
        del values, expr
        ops.release_workspaces()
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
