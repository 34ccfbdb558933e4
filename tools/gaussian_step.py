#!/usr/bin/env python3
"""Time the Gaussian factor step (exact expected log-likelihood + the five gradients) on one GPU, in one process: the fused
gpz_gaussian_fa, its value-only form, and the torch composition of the same closed form (forward + backward through
autograd, which materialises the (D, N) residual and its scaled copy), at the Slide-seq mini-batch (D = 17702,
N_b = 7000, 20 factors) and the published benchmark shape (D = 80, N = 1037, L = 4).  The arms alternate round by round
after a warm-up; the median (and minimum) of --reps rounds (>= 30) is reported; peak temporary memory is the allocator's
high-water mark above what is live before the call.  ``two_reads_of_y_ms`` is the time to read y twice at the HBM copy
rate DESIGN.md section 7 records for this chip (5.43 TB/s).  One JSON line per shape.

    python tools/gaussian_step.py [--reps 30] [--shape slideseq|benchmark|all]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402

SHAPES = {"slideseq": dict(D=17702, N=7000, Lt=20), "benchmark": dict(D=80, N=1037, Lt=4)}
COPY_RATE = 5.43e12          # bytes / s, DESIGN.md section 7


def inputs(D, N, Lt, dev):
    g = torch.Generator().manual_seed(1)
    mean = 0.8 * torch.randn(Lt, N, generator=g)
    scale = 0.2 + 0.3 * torch.rand(Lt, N, generator=g)
    W = torch.randn(D, Lt, generator=g)
    b = 2.0 * torch.randn(D, generator=g)
    sd = torch.logspace(math.log10(0.05), math.log10(3.0), D)
    y = b[:, None] + W @ (mean + scale * torch.randn(Lt, N, generator=g)) + 1.5 * sd[:, None] * torch.randn(D, N, generator=g)
    return [t.to(dev) for t in (mean, scale, W, b, sd, y)]


def torch_step(mean, scale, W, b, sd, y):
    lv = [t.clone().requires_grad_(True) for t in (mean, scale, W, b, sd)]
    m, s, w, bb, sg = lv
    ll = torch.distributions.Normal(bb[:, None] + w @ m, sg[:, None], validate_args=False).log_prob(y).sum() \
        - 0.5 * ((w ** 2 / (sg ** 2)[:, None]) @ s ** 2).sum()
    ll.backward()
    return (ll.detach(), *(t.grad for t in lv))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shape", default="all", choices=["all", *SHAPES])
    a = ap.parse_args()
    reps = max(a.reps, 30)
    dev = torch.device("cuda")
    for name, sh in SHAPES.items():
        if a.shape not in ("all", name):
            continue
        t = inputs(dev=dev, **sh)
        arms = {"fused": lambda: ops.gaussian_fa(*t), "value_only": lambda: ops.gaussian_fa(*t, grads=False),
                "torch": lambda: torch_step(*t)}
        ms, peak, out = measure(arms, reps)
        y_bytes = 4 * sh["D"] * sh["N"]
        ref, got = out["torch"], out["fused"]
        grad_err = max(float((g.double() - r.double()).abs().max() / (r.double().abs().max() + 1e-30))
                       for g, r in zip(got[2:], ref[1:]))
        res = dict(shape=name, **sh, reps=reps,
                   fused_ms=round(ms["fused"][0], 4), fused_min_ms=round(ms["fused"][1], 4),
                   value_only_ms=round(ms["value_only"][0], 4), torch_ms=round(ms["torch"][0], 4),
                   torch_min_ms=round(ms["torch"][1], 4), torch_over_fused=round(ms["torch"][0] / ms["fused"][0], 2),
                   two_reads_of_y_ms=round(2e3 * y_bytes / COPY_RATE, 4),
                   fused_over_two_reads=round(ms["fused"][0] / (2e3 * y_bytes / COPY_RATE), 2),
                   fused_peak_temp_mib=round(peak["fused"], 1), torch_peak_temp_mib=round(peak["torch"], 1),
                   partials_mib=round(ops.gaussian_fa_plan(sh["N"], sh["D"], sh["Lt"])["partials_bytes"] / 2 ** 20, 1),
                   y_mib=round(y_bytes / 2 ** 20, 1), fused_loglik=float(got[0]), torch_loglik=float(ref[0]),
                   max_grad_err_over_max_grad=grad_err)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
