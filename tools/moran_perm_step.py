#!/usr/bin/env python3
"""Time the permutation null of Moran's I (gpz_gene_morans_perm_sparse, gpz_morans_perm_rows) on one GPU, in one process, at
the Slide-seq shape (D = 17702 genes, N = 39694 spots, K = 6 neighbours, P = 100 permutations) at 1 / 5 / 20 % density:
  perm_global   the sparse entry, the gene's line in the scratch memory (line_mode 1)
  perm_lds      the sparse entry, the line in LDS (line_mode 2)
  perm_rows     the dense-rows entry on the densified (D, N) array, line_mode as the plan chooses (--rows-at: at 20 % only
                by default; its time does not depend on the density)
  yardstick     what a user composes without them: P calls of ``ops.gene_morans_i_sparse`` on tables relabelled with torch
                indexing (T_pi[pi] = pi[nbr]), one synchronisation each
The arms alternate round by round after a warm-up; the median (and minimum) of --reps rounds (>= 30) is reported, with the
line gathers per second (stored entries x K x P / time), the density at which the dense-rows entry would cross the sparse
one, and whether the arms agree.  One JSON line per density.

    python tools/moran_perm_step.py [--reps 30] [--density 0.01 0.05 0.2] [--perms 100] [--json FILE]"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd.likelihoods import SparseCounts  # noqa: E402


def sparse_counts(D, N, density, dev):
    """Counts of 1 .. 8 at ``density`` of the positions, drawn on the device."""
    g = torch.Generator(device=dev).manual_seed(1)
    counts = torch.rand(D, N, generator=g, device=dev)
    counts = (counts < density) * (1.0 + torch.floor(8.0 * torch.rand(D, N, generator=g, device=dev)))
    return SparseCounts(counts)


def yardstick(c, nbr, perms):
    """(D, P) simulated I from the entry without permutations: one relabelled table and one call per permutation."""
    out = []
    for pi in perms.long():
        T = torch.empty_like(nbr)
        T[pi] = pi[nbr]
        out.append(ops.gene_morans_i_sparse(c, T))
    return torch.stack(out, dim=1)


def measure(arms, reps, warmup=2):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out, ts = {}, {k: [] for k in arms}
    for k, fn in arms.items():
        for _ in range(warmup):
            out[k] = fn()
    torch.cuda.synchronize()
    for i in range(reps):
        for k, fn in arms.items():
            ev0.record(); out[k] = fn(); ev1.record(); torch.cuda.synchronize()
            ts[k].append(ev0.elapsed_time(ev1))
        if i % 10 == 0:
            print(f"round {i}: " + ", ".join(f"{k} {v[-1]:.1f} ms" for k, v in ts.items()), file=sys.stderr, flush=True)
    return {k: (statistics.median(v), min(v)) for k, v in ts.items()}, out


def run(D, N, K, P, density, reps, with_rows, dev):
    gc.collect()
    torch.cuda.empty_cache()
    c = sparse_counts(D, N, density, dev)
    X = torch.rand(N, 2, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(dev)
    nbr = ops.spatial_knn(X, K)
    g = torch.Generator(device=dev).manual_seed(3)
    perms = torch.stack([torch.randperm(N, generator=g, device=dev) for _ in range(P)]).to(torch.int32)
    arms = {"perm_global": lambda: ops.gene_morans_perm_sparse(c, nbr, perms, return_sims=True, line_mode="global"),
            "perm_lds": lambda: ops.gene_morans_perm_sparse(c, nbr, perms, return_sims=True, line_mode="lds"),
            "yardstick": lambda: yardstick(c, nbr, perms)}
    if with_rows:
        dense = c.to_dense()
        arms["perm_rows"] = lambda: ops.morans_perm_rows(dense, nbr, perms, return_sims=True)
    ms, out = measure(arms, reps)
    plan = ops.morans_perm_plan(N, D, K, P, nnz=c.nnz)
    res = dict(D=D, N=N, K=K, P=P, density=density, nnz=c.nnz, reps=reps, perm_batch=plan["perm_batch"],
               auto_line_mode=plan["line_mode"], scratch_mib=round(plan["partials_bytes"] / 2 ** 20, 1))
    for k in arms:
        res[k + "_ms"] = round(ms[k][0], 3)
        res[k + "_min_ms"] = round(ms[k][1], 3)
        res[k + "_gathers_per_s"] = float(f"{(D * N if k == 'perm_rows' else c.nnz) * K * P / (ms[k][0] * 1e-3):.4g}")
    a, b, y = out["perm_global"], out["perm_lds"], out["yardstick"]
    same = lambda s, t: bool(torch.equal(torch.nan_to_num(s, nan=-7.0), torch.nan_to_num(t, nan=-7.0)))  # noqa: E731
    res.update(global_over_yardstick=round(ms["perm_global"][0] / ms["yardstick"][0], 3),
               lds_over_yardstick=round(ms["perm_lds"][0] / ms["yardstick"][0], 3),
               lds_over_global=round(ms["perm_lds"][0] / ms["perm_global"][0], 3),
               modes_same_bits=all(same(getattr(a, f), getattr(b, f)) for f in ("I", "sims", "sim_mean", "sim_m2"))
               and bool(torch.equal(a.n_ge, b.n_ge) and torch.equal(a.n_le, b.n_le)),
               sims_same_bits_as_yardstick=same(a.sims, y))
    if with_rows:
        r = out["perm_rows"]
        ok = ~(torch.isnan(a.sims) | torch.isnan(r.sims))
        res.update(rows_max_abs_diff=float((a.sims - r.sims)[ok].abs().max()),
                   rows_counts_equal=bool(torch.equal(a.n_ge, r.n_ge) and torch.equal(a.n_le, r.n_le)),
                   crossing_density=round(density * ms["perm_rows"][0] / min(ms["perm_global"][0], ms["perm_lds"][0]), 3))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--density", type=float, nargs="+", default=[0.01, 0.05, 0.2])
    ap.add_argument("--rows-at", type=float, nargs="*", default=[0.2], help="densities at which the dense-rows entry runs too")
    ap.add_argument("--genes", type=int, default=17702)
    ap.add_argument("--spots", type=int, default=39694)
    ap.add_argument("--neighbours", type=int, default=6)
    ap.add_argument("--perms", type=int, default=100)
    ap.add_argument("--json", default=None, help="append the result lines to this file too")
    a = ap.parse_args()
    dev = torch.device("cuda")
    for density in a.density:
        res = run(a.genes, a.spots, a.neighbours, a.perms, density, max(a.reps, 30), density in a.rows_at, dev)
        if a.json:
            with open(a.json, "a") as f:
                f.write(json.dumps(res) + "\n")
        ops.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
