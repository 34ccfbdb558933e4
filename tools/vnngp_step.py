#!/usr/bin/env python3
"""Time VNNGP (NSF_benchmarks.ipynb shape: K=10 neighbours, M=1000 inducing points, Slide-seq-sized N)
through the gpzoo module: forward only, and forward + loss.backward() with every parameter trainable.

    python tools/vnngp_step.py [--kernel {rbf,matern12,matern32,matern52}] [--reps R]

``--kernel``: the covariance (default rbf: NSF_RBF, as before; the Matern kinds are the batched_Matern* classes with
length-L parameters).  The headline figures are the minimum over the timed repetitions as before; the median and the
min..max range of the same repetitions follow (the first repetition is warm-up and not counted).  Per-kernel times:
run this under ``rocprofv3 --kernel-trace --stats -- python3 tools/vnngp_step.py ...``."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn as nn
from torch import distributions

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo.gp import VNNGP  # noqa: E402
import gpzoo.kernels as gk  # noqa: E402


def make_kernel(name, L):
    if name == "rbf":
        return gk.NSF_RBF(sigma=1.0, lengthscale=8.0, L=L)
    k = dict(matern12=gk.batched_Matern12, matern32=gk.batched_Matern32, matern52=gk.batched_Matern52)[name]()
    k.sigma = nn.Parameter(torch.ones(L))
    k.lengthscale = nn.Parameter(8.0 * torch.ones(L))
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", choices=["rbf", "matern12", "matern32", "matern52"], default="rbf")
    ap.add_argument("--reps", type=int, default=6, help="repetitions per figure, the first one not counted")
    args = ap.parse_args()
    torch.manual_seed(0)
    N, M, L, K = 40000, 1000, 10, 10
    dev = torch.device("cuda")
    X = (torch.rand(N, 2) * 200 - 100).to(dev)
    y = torch.randn(L, N, device=dev)
    gp = VNNGP(make_kernel(args.kernel, L), dim=2, M=M, K=K, jitter=1e-2)
    gp.Z = nn.Parameter(X[torch.randperm(N)[:M]].clone().cpu())
    gp.mu = nn.Parameter(torch.zeros(L, M))
    gp.Lu = nn.Parameter(0.01 * torch.randn(L, M, M))
    gp = gp.to(dev)

    def timed(fn, reps=max(args.reps, 2)):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts = [1e3 * t for t in ts[1:]]
        return min(ts), statistics.median(ts), max(ts)

    def fwd():
        with torch.no_grad():
            gp(X)

    def step():
        gp.zero_grad()
        qF, qU, pU = gp(X)
        loss = -(distributions.Normal(qF.mean, 0.5).log_prob(y).sum() - (qF.scale ** 2).sum() / 0.5
                 - distributions.kl_divergence(qU, pU).sum())
        loss.backward()

    f, s = timed(fwd), timed(step)
    tag = "" if args.kernel == "rbf" else f" {args.kernel}"
    print(f"VNNGP N={N} M={M} L={L} K={K} f32{tag}: forward {f[0]:.2f} ms, forward+backward (all parameters) {s[0]:.2f} ms"
          f" [median {f[1]:.2f} / {s[1]:.2f} ms, range {f[0]:.2f}..{f[2]:.2f} / {s[0]:.2f}..{s[2]:.2f} ms over "
          f"{max(args.reps, 2) - 1} repetitions]")


if __name__ == "__main__":
    main()
