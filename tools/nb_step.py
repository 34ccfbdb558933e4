#!/usr/bin/env python3
"""Time the negative-binomial NSF step (expected log-likelihood + the five gradients) on one GPU, in one process:
the fused gpz_nb_nsf, the fused Poisson step on the same inputs (ops.poisson_nsf) and the torch composition of the NB step
(forward + backward through NegativeBinomial.log_prob on the (E, D, N) rate), at the two shapes the README quotes for the
Poisson step -- the Slide-seq mini-batch (D = 17702, N_b = 7000, 20 factors, E = 3) and the published benchmark
(N = 1037, D = 80, L = 4, E = 20).  Warm-up, then the median of --reps repetitions (>= 30); peak temporary memory is the
allocator's high-water mark above what is live before the call.  One JSON line per shape.

    python tools/nb_step.py [--reps 30] [--shape slideseq|benchmark|all] [--no-torch]"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402

SHAPES = {"slideseq": dict(D=17702, N=7000, Lt=20, E=3), "benchmark": dict(D=80, N=1037, Lt=4, E=20)}


def inputs(D, N, Lt, E, dev):
    g = torch.Generator().manual_seed(1)
    rng = np.random.default_rng(1)
    mean = (0.3 * torch.randn(Lt, N, generator=g)).to(dev)
    scale = (0.2 + 0.3 * torch.rand(Lt, N, generator=g)).to(dev)
    eps = torch.randn(E, Lt, N, generator=g).to(dev)
    W = (torch.rand(D, Lt, generator=g) + 0.05).to(dev)
    V = (0.5 + torch.rand(N, generator=g)).to(dev)
    theta = torch.logspace(math.log10(0.3), math.log10(50.0), D)
    shape = theta.double().numpy()[:, None]
    rate = 0.3 + 1.7 * rng.random((D, N), dtype=np.float32)
    y = torch.from_numpy(rng.poisson(rng.gamma(shape, rate / shape)).astype(np.float32)).to(dev)
    return mean, scale, eps, W, V, theta.to(dev), y


def timed(fn, reps, warmup=3):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(reps):
        ev0.record(); out = fn(); ev1.record(); torch.cuda.synchronize()
        ts.append(ev0.elapsed_time(ev1))
    return statistics.median(ts), (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shape", default="all", choices=["all", *SHAPES])
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition (it holds several (E, D, N) arrays)")
    a = ap.parse_args()
    reps = max(a.reps, 30)
    dev = torch.device("cuda")
    for name, sh in SHAPES.items():
        if a.shape not in ("all", name):
            continue
        mean, scale, eps, W, V, theta, y = inputs(dev=dev, **sh)
        t_nb, m_nb, out = timed(lambda: ops.nb_nsf(mean, scale, eps, W, V, theta, y), reps)
        t_po, m_po, _ = timed(lambda: ops.poisson_nsf(mean, scale, eps, W, V, y), reps)
        res = dict(shape=name, **sh, reps=reps, nb_ms=round(t_nb, 4), poisson_ms=round(t_po, 4), nb_over_poisson=round(t_nb / t_po, 3),
                   nb_peak_temp_mib=round(m_nb, 1), poisson_peak_temp_mib=round(m_po, 1), nb_loglik=float(out[0]),
                   nb_workspace_mib=round(ops.nb_nsf_plan(sh["N"], sh["D"], sh["Lt"], sh["E"])["workspace_bytes"] / 2 ** 20, 1))
        if not a.no_torch:
            def torch_path():
                lv = [t.clone().requires_grad_(True) for t in (mean, scale, W, V, theta)]
                rate = lv[3] * torch.matmul(lv[2], torch.exp(lv[0] + lv[1] * eps))
                th = lv[4][:, None]
                ll = torch.distributions.NegativeBinomial(total_count=th, logits=torch.log(rate) - torch.log(th),
                                                          validate_args=False).log_prob(y).mean(0).sum()
                ll.backward()
                return ll.detach()
            t_t, m_t, ref = timed(torch_path, reps)
            res.update(torch_ms=round(t_t, 4), torch_over_nb=round(t_t / t_nb, 2), torch_peak_temp_mib=round(m_t, 1),
                       torch_loglik=float(ref))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
