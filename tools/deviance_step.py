#!/usr/bin/env python3
"""Time the Poisson deviance entries (ops.poisson_deviance, ops.poisson_deviance_sparse) on one MI355X next to the torch
composition that materialises the (D, B) rate, on the same inputs in the same process: median of 20 calls after warm-up,
synthetic counts, Lt = 20 factors, at

  batch   D = 17 702 genes, B = 7000 of N = 39 694 spots    dense entry on y[:, idx]; sparse entry on the view at 1 / 5 / 20 %
  full    D = 17 702, all 39 694 spots                      sparse entry at 5 %; the torch composition where it fits

Reported per point: milliseconds, the dense entry's share of one read of y (D B 4 bytes) as GB/s, the workspace of each
entry, and the torch composition's time and peak memory above its inputs.

    python tools/deviance_step.py [--json FILE] [--quick]

``--quick`` runs the batch shape at 5 % only."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd.likelihoods import SparseCounts  # noqa: E402

N_ALL, B, D, LT = 39694, 7000, 17702, 20
REPS, WARM = 20, 3


def median_ms(fn, reps=REPS, warm=WARM):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def synthetic_counts(D, N, density, dev, seed):
    """(D, N) fp32 counts on the device, built in column blocks so that no temporary is larger than the result."""
    g = torch.Generator(device=dev).manual_seed(seed)
    y = torch.empty((D, N), dtype=torch.float32, device=dev)
    for n0 in range(0, N, 4096):
        n1 = min(N, n0 + 4096)
        keep = torch.rand((D, n1 - n0), generator=g, device=dev) < density
        y[:, n0:n1] = (torch.poisson(torch.full((D, n1 - n0), 2.0, device=dev), generator=g) + 1.0) * keep
    return y


def torch_composition(mean, scale, W, V, y):
    """What a user composes from the rate: every element-wise step is a (D, B) temporary."""
    mu = V * torch.matmul(W, torch.exp(mean + 0.5 * scale * scale))
    dev = 2.0 * (torch.xlogy(y, y / mu) - y + mu)
    r = y.sum(1, dtype=torch.float64) / V.sum(dtype=torch.float64)
    mu0 = V * r[:, None].float()
    null = 2.0 * (torch.where(y > 0, y * torch.log(y / mu0), torch.zeros_like(y)) - y + mu0)
    return (dev.sum(1, dtype=torch.float64), dev.sum(0, dtype=torch.float64), null.sum(1, dtype=torch.float64),
            y.sum(dtype=torch.float64), mu.sum(dtype=torch.float64))


def torch_point(mean, scale, W, V, y):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    try:
        ms = median_ms(lambda: torch_composition(mean, scale, W, V, y), reps=5, warm=1)
    except torch.cuda.OutOfMemoryError:
        return None, None
    return ms, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def params(n, dev):
    g = torch.Generator().manual_seed(1)
    return ((0.3 * torch.randn(LT, n, generator=g)).to(dev), (0.2 + 0.3 * torch.rand(LT, n, generator=g)).to(dev),
            (torch.rand(D, LT, generator=g) + 0.05).to(dev), (0.5 + torch.rand(n, generator=g)).to(dev))


def main():
    args = sys.argv[1:]
    out = None
    if "--json" in args:
        i = args.index("--json")
        out = args[i + 1]
        del args[i:i + 2]
    quick = "--quick" in args
    dev = torch.device("cuda")
    rows = []
    g = torch.Generator().manual_seed(2)
    idx = torch.randperm(N_ALL, generator=g)[:B].to(dev)
    pb, pf = params(B, dev), params(N_ALL, dev)
    for density in ((0.05,) if quick else (0.01, 0.05, 0.20)):
        y = synthetic_counts(D, N_ALL, density, dev, seed=int(1000 * density))
        s = SparseCounts(y)
        view = s[:, idx]
        yb = y[:, idx].contiguous()
        rec = dict(shape="batch", D=D, B=B, N=N_ALL, Lt=LT, density=density, nnz=s.nnz, nnz_batch=view.nnz,
                   dense_workspace_bytes=ops.poisson_deviance_plan(B, D, LT)["workspace_bytes"],
                   sparse_workspace_bytes=ops.poisson_deviance_sparse_plan(N_ALL, B, D, LT, s.nnz)["workspace_bytes"])
        rec["dense_ms"] = median_ms(lambda: ops.poisson_deviance(*pb, yb))
        rec["dense_GBps_of_y"] = D * B * 4 / rec["dense_ms"] / 1e6
        rec["sparse_ms"] = median_ms(lambda: ops.poisson_deviance_sparse(*pb, view))
        a, b = ops.poisson_deviance(*pb, yb), ops.poisson_deviance_sparse(*pb, view)
        rec["total_dense"], rec["total_sparse"] = float(a["total"]), float(b["total"])
        if density == 0.05:
            rec["torch_ms"], rec["torch_peak_MiB"] = torch_point(*pb, yb)
            t = torch_composition(*pb, yb)
            rec["total_torch"] = float(t[0].sum())
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        if density == 0.05 and not quick:
            full = dict(shape="full", D=D, B=N_ALL, N=N_ALL, Lt=LT, density=density, nnz=s.nnz,
                        sparse_workspace_bytes=ops.poisson_deviance_sparse_plan(N_ALL, N_ALL, D, LT, s.nnz)["workspace_bytes"])
            full["sparse_ms"] = median_ms(lambda: ops.poisson_deviance_sparse(*pf, s))
            full["dense_ms"] = median_ms(lambda: ops.poisson_deviance(*pf, y), reps=5, warm=1)
            full["dense_GBps_of_y"] = D * N_ALL * 4 / full["dense_ms"] / 1e6
            full["torch_ms"], full["torch_peak_MiB"] = torch_point(*pf, y)
            full["total_sparse"] = float(ops.poisson_deviance_sparse(*pf, s)["total"])
            full["total_dense"] = float(ops.poisson_deviance(*pf, y)["total"])
            rows.append(full)
            print(json.dumps(full), flush=True)
        del y, s, view, yb
        torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
