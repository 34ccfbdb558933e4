#!/usr/bin/env python3
"""Time the sparse Gaussian factor step (gpz_gaussian_fa_sparse on a ``SparseExpression``) against the dense one
(gpz_gaussian_fa on the dense array) on one GPU, in one process, at the Slide-seq mini-batch (D = 17702 genes, N = 39694
spots, a batch of 7000, 20 factors) at 1 / 5 / 20 % density and at the published benchmark shape (D = 80, N = 1037, L = 4,
the whole data set as the batch).  What a mini-batch step pays in each form:
  sparse_view_step   the no-copy view ``expr[:, idx]`` (its index check deferred as in the training loops) + the sparse step
  dense_gather_step  the gather ``y[:, idx]`` of the dense array + the dense step
and the bare steps on a prepared view / a prepared (D, B) array, and the gather alone.  The arms alternate round by round
after a warm-up; the median (and minimum) of --reps rounds (>= 30) is reported.  Memory: the bytes y holds in each form
and the allocator's high-water mark above what is live before the call.  One JSON line per shape and density.

    python tools/sparse_gaussian_step.py [--reps 30] [--shape slideseq|benchmark|all] [--density 0.01 0.05 0.2]"""
import argparse
import gc
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd.likelihoods import SparseCounts  # noqa: E402
from gpzoo_amd.utilities import log_normalize  # noqa: E402

SHAPES = {"slideseq": dict(D=17702, N=39694, B=7000, Lt=20), "benchmark": dict(D=80, N=1037, B=1037, Lt=4)}


def expression(D, N, density, dev):
    """Counts of 1 .. 8 at ``density`` of the positions, drawn on the device, and their centred log-normalisation."""
    g = torch.Generator(device=dev).manual_seed(1)
    counts = torch.rand(D, N, generator=g, device=dev)
    counts = (counts < density) * (1.0 + torch.floor(8.0 * torch.rand(D, N, generator=g, device=dev)))
    sc = SparseCounts(counts)
    del counts
    return log_normalize(sc)


def parameters(D, B, Lt, dev):
    g = torch.Generator().manual_seed(2)
    mean = 0.8 * torch.randn(Lt, B, generator=g)
    scale = 0.2 + 0.3 * torch.rand(Lt, B, generator=g)
    W = torch.randn(D, Lt, generator=g) / Lt ** 0.5
    b = 0.1 * torch.randn(D, generator=g)
    sd = torch.logspace(math.log10(0.05), math.log10(3.0), D)
    return [t.to(dev) for t in (mean, scale, W, b, sd)]


def measure(arms, reps, warmup=3):
    """Median / minimum milliseconds and peak temporary MiB per arm, the arms alternating within every round."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out, ts, peak = {}, {k: [] for k in arms}, {}
    for k, fn in arms.items():
        for _ in range(warmup):
            out[k] = fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out[k] = fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    for _ in range(reps):
        for k, fn in arms.items():
            ev0.record(); out[k] = fn(); ev1.record(); torch.cuda.synchronize()
            ts[k].append(ev0.elapsed_time(ev1))
    return {k: (statistics.median(v), min(v)) for k, v in ts.items()}, peak, out


def sparse_bytes(expr):
    v = expr.values
    return sum(getattr(v, k).numel() * getattr(v, k).element_size() for k in v._PARTS) + 8 * expr.offset.numel()


def run(name, D, N, B, Lt, density, reps, dev):
    gc.collect()                               # the previous run's arrays (held by its closures) are gone before any is measured
    torch.cuda.empty_cache()
    expr = expression(D, N, density, dev)
    dense = expr.to_dense()
    p = parameters(D, B, Lt, dev)
    batch = B < N
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(3))[:B].to(dev) if batch else None
    view = expr[:, idx] if batch else expr
    yb = dense[:, idx] if batch else dense

    def sparse_view_step():
        with ops.deferred_info():
            return ops.gaussian_fa_sparse(*p, expr[:, idx] if batch else expr)
    arms = {"sparse_view_step": sparse_view_step,
            "dense_gather_step": lambda: ops.gaussian_fa(*p, dense[:, idx] if batch else dense),
            "sparse_step": lambda: ops.gaussian_fa_sparse(*p, view),
            "dense_step": lambda: ops.gaussian_fa(*p, yb),
            "sparse_value_only": lambda: ops.gaussian_fa_sparse(*p, view, grads=False)}
    if batch:
        arms["gather"] = lambda: dense[:, idx]
    ms, peak, out = measure(arms, reps)
    sp, de = out["sparse_step"], out["dense_step"]
    grad_err = max(float((g.double() - r.double()).abs().max() / (r.double().abs().max() + 1e-30))
                   for g, r in zip(sp[3:], de[2:]))
    plan = ops.gaussian_fa_sparse_plan(N, B, D, Lt, expr.nnz)
    res = dict(shape=name, D=D, N=N, B=B, Lt=Lt, density=density, nnz=expr.nnz, reps=reps)
    for k in arms:
        res[k + "_ms"] = round(ms[k][0], 4)
        res[k + "_min_ms"] = round(ms[k][1], 4)
    res.update(view_step_over_gather_step=round(ms["sparse_view_step"][0] / ms["dense_gather_step"][0], 3),
               sparse_over_dense_bare=round(ms["sparse_step"][0] / ms["dense_step"][0], 3),
               y_dense_mib=round(4 * D * N / 2 ** 20, 1), y_sparse_mib=round(sparse_bytes(expr) / 2 ** 20, 1),
               sparse_view_step_peak_temp_mib=round(peak["sparse_view_step"], 1),
               dense_gather_step_peak_temp_mib=round(peak["dense_gather_step"], 1),
               sparse_scratch_mib=round(plan["workspace_bytes"] / 2 ** 20, 1),
               dense_partials_mib=round(ops.gaussian_fa_plan(B, D, Lt)["partials_bytes"] / 2 ** 20, 1),
               sparse_loglik=float(sp[0]), dense_loglik=float(de[0]), max_grad_err_over_max_grad=grad_err)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shape", default="all", choices=["all", *SHAPES])
    ap.add_argument("--density", type=float, nargs="+", default=[0.01, 0.05, 0.2])
    a = ap.parse_args()
    reps = max(a.reps, 30)
    dev = torch.device("cuda")
    for name, sh in SHAPES.items():
        if a.shape not in ("all", name):
            continue
        for density in a.density:
            run(name, density=density, reps=reps, dev=dev, **sh)
            ops.release_workspaces()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
