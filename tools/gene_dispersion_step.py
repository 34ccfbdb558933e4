#!/usr/bin/env python3
"""Time the gene-wise dispersion fit of a ``SparseCounts`` (gpz_gene_dispersion_sparse) on one GPU, in one process, at the
Slide-seq shape (D = 17702 genes, N = 39694 spots) at 1 / 5 / 20 % density, with the spots' totals as sizes (every score
evaluation sweeps the N sizes) and with constant sizes (the all-spot sums are N f(x)), against what a user composes
without it:
  torch            the same equations as torch ops on dense fp64 chunks of ``--chunk`` genes (digamma / polygamma for the
                   sums over k, log1p for the zero part): the moment start and as many Newton steps in log theta, all genes
                   in step, as the kernel's mean evaluations per gene, rounded up.  The dense (D, N) array it reads is
                   made before the clock starts.
The arms alternate round by round after a warm-up; the median (and minimum) of --reps rounds (>= 30) is reported, with the
mean score evaluations per gene and the evaluated terms per second (one term = one spot, or one stored entry, of one score
or gain evaluation).  One JSON line per density and kind of sizes.

    python tools/gene_dispersion_step.py [--reps 30] [--density 0.01 0.05 0.2] [--genes 17702 --spots 39694] [--no-torch]"""
import argparse
import gc
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gene_rank_step import measure, sparse_counts  # noqa: E402
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd.utilities import _spot_totals_tensor  # noqa: E402

THETA_RANGE = (1e-4, 1e6)


def dispersion_torch(dense, size, n_eval, chunk):
    """log theta of every gene after the moment start and ``n_eval`` Newton steps in t = log theta, clamped into the range."""
    t_lo, t_hi = math.log(THETA_RANGE[0]), math.log(THETA_RANGE[1])
    S2, total = (size * size).sum(), size.sum()
    out = []
    for lo in range(0, dense.shape[0], chunk):
        y = dense[lo:lo + chunk].to(torch.float64)
        sy = y.sum(dim=1, keepdim=True)
        p = sy / total
        mu = p * size[None, :]
        num = p * p * S2
        den = ((y - mu) ** 2).sum(dim=1, keepdim=True) - sy
        t = torch.log(torch.where(den > 0, num / den, torch.full_like(den, THETA_RANGE[1])).clamp(*THETA_RANGE))
        for _ in range(n_eval):
            th = torch.exp(t)
            x, tm = mu / th, th + mu
            q = x / (1.0 + x)
            S = th * (torch.digamma(y + th) - torch.digamma(th) - y / tm + q - torch.log1p(x)).sum(dim=1, keepdim=True)
            dS = S + th * th * (torch.polygamma(1, y + th) - torch.polygamma(1, th) + y / (tm * tm)).sum(dim=1, keepdim=True) \
                + th * (q * q).sum(dim=1, keepdim=True)
            t = torch.where(dS < 0, t - S / dS, t - 1.0).clamp(t_lo, t_hi)
        out.append(t[:, 0])
    return torch.cat(out)


def run(D, N, density, sizes, reps, chunk, with_torch, dev):
    gc.collect()
    torch.cuda.empty_cache()
    c = sparse_counts(D, N, density, dev)
    size = _spot_totals_tensor(c).clamp_min(1.0) if sizes == "totals" else torch.ones(N, dtype=torch.float64, device=dev)
    theta, gain, pl, status, iterations = ops.gene_dispersion_sparse(c, size, *THETA_RANGE)
    evals = (iterations + (status != 4) * 2 + ((status == 0) | (status == 2) | (status == 3))).double()   # ends, steps, gain
    mean_it = float(iterations[status == 0].double().mean()) if bool((status == 0).any()) else 0.0
    arms = {"hip": lambda: ops.gene_dispersion_sparse(c, size, *THETA_RANGE)[0]}
    if with_torch:
        dense = c.to_dense()
        n_eval = int(math.ceil(mean_it)) + 2
        arms["torch"] = lambda: dispersion_torch(dense, size, n_eval, chunk)
    ms, out = measure(arms, reps)
    nnz_d = (c.row_ptr[1:] - c.row_ptr[:-1]).double()
    spot_terms = float(evals.sum()) * N if sizes == "totals" else 0.0
    entry_terms = float((evals * nnz_d).sum())
    res = dict(D=D, N=N, density=density, sizes=sizes, nnz=c.nnz, reps=reps, hip_ms=round(ms["hip"][0], 3),
               hip_min_ms=round(ms["hip"][1], 3), mean_iterations=round(mean_it, 2), max_iterations=int(iterations.max()),
               status_counts=torch.bincount(status.long(), minlength=5).tolist(),
               spot_terms_per_s=round(spot_terms / (ms["hip"][0] * 1e-3), 0), entry_terms_per_s=round(entry_terms / (ms["hip"][0] * 1e-3), 0))
    if with_torch:
        ok = status == 0
        res.update(torch_ms=round(ms["torch"][0], 3), torch_min_ms=round(ms["torch"][1], 3), torch_evaluations=n_eval,
                   hip_over_torch=round(ms["hip"][0] / ms["torch"][0], 4),
                   max_abs_diff_log_theta=float((torch.log(out["hip"][ok]) - out["torch"][ok]).abs().max()))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--density", type=float, nargs="+", default=[0.01, 0.05, 0.2])
    ap.add_argument("--genes", type=int, default=17702)
    ap.add_argument("--spots", type=int, default=39694)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    for density in a.density:
        for sizes in ("totals", "constant"):
            run(a.genes, a.spots, density, sizes, max(a.reps, 30), a.chunk, not a.no_torch, dev)
            ops.release_workspaces()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
