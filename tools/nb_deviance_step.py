#!/usr/bin/env python3
"""Time the NB deviance entries (ops.nb_deviance, ops.nb_deviance_sparse) on one MI355X next to the Poisson deviance entry
and to the torch composition through NegativeBinomial.log_prob, on the same inputs in the same process: median of 30 calls
after warm-up, synthetic counts at the Slide-seq mini-batch, D = 17 702 genes, B = 7000 spots, Lt = 20 factors, theta
log-spaced over [0.3, 50] across the genes, at 1 / 5 / 20 % non-zeros.

Reported per density: milliseconds of the dense NB entry, of the dense Poisson entry and their ratio, of the sparse NB entry
and of the sparse Poisson entry, the workspace of each NB entry, and (at 5 %) the torch composition's time and peak memory
above its inputs.

    python tools/nb_deviance_step.py [--json FILE] [--quick]

``--quick`` runs 5 % only."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd.likelihoods import SparseCounts  # noqa: E402

B, D, LT = 7000, 17702, 20
REPS, WARM = 30, 3


def median_ms(fn, reps=REPS, warm=WARM):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def synthetic_counts(density, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    keep = torch.rand((D, B), generator=g, device=dev) < density
    return (torch.poisson(torch.full((D, B), 2.0, device=dev), generator=g) + 1.0) * keep


def torch_composition(mean, scale, W, V, theta, y):
    """What a user composes from the rate: every element-wise step is a (D, B) temporary."""
    NB, P = torch.distributions.NegativeBinomial, torch.distributions.Poisson
    th = theta[:, None]
    mu = V * torch.matmul(W, torch.exp(mean + 0.5 * scale * scale))

    def nb(m):
        return NB(total_count=th, logits=torch.log(m) - torch.log(th), validate_args=False)
    ll = nb(mu).log_prob(y)
    sat = torch.where(y > 0, nb(torch.where(y > 0, y, torch.ones_like(y))).log_prob(y), torch.zeros_like(y))
    dev = 2.0 * (sat - ll)
    r = y.sum(1, dtype=torch.float64) / V.sum(dtype=torch.float64)
    mu0 = torch.where(r[:, None] > 0, V * r[:, None].float(), torch.ones_like(mu))
    null = 2.0 * (sat - nb(mu0).log_prob(y))
    pll = P(mu, validate_args=False).log_prob(y)
    f64 = torch.float64
    return (dev.sum(1, dtype=f64), dev.sum(0, dtype=f64), null.sum(1, dtype=f64), ll.sum(1, dtype=f64), ll.sum(0, dtype=f64),
            pll.sum(1, dtype=f64), y.sum(dtype=f64), mu.sum(dtype=f64))


def torch_point(*args):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    try:
        ms = median_ms(lambda: torch_composition(*args), reps=5, warm=1)
    except torch.cuda.OutOfMemoryError:
        return None, None
    return ms, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def params(dev):
    g = torch.Generator().manual_seed(1)
    return ((0.3 * torch.randn(LT, B, generator=g)).to(dev), (0.2 + 0.3 * torch.rand(LT, B, generator=g)).to(dev),
            (torch.rand(D, LT, generator=g) + 0.05).to(dev), (0.5 + torch.rand(B, generator=g)).to(dev))


def main():
    args = sys.argv[1:]
    out = None
    if "--json" in args:
        i = args.index("--json")
        out = args[i + 1]
        del args[i:i + 2]
    quick = "--quick" in args
    dev = torch.device("cuda")
    p = params(dev)
    theta = torch.logspace(-0.5228787, 1.69897, D, device=dev)
    rows = []
    for density in ((0.05,) if quick else (0.01, 0.05, 0.20)):
        y = synthetic_counts(density, dev, seed=int(1000 * density))
        s = SparseCounts(y)
        rec = dict(D=D, B=B, Lt=LT, density=density, nnz=s.nnz,
                   dense_workspace_bytes=ops.nb_deviance_plan(B, D, LT)["workspace_bytes"],
                   sparse_workspace_bytes=ops.nb_deviance_sparse_plan(B, B, D, LT, s.nnz)["workspace_bytes"])
        rec["nb_dense_ms"] = median_ms(lambda: ops.nb_deviance(*p, theta, y))
        rec["poisson_dense_ms"] = median_ms(lambda: ops.poisson_deviance(*p, y))
        rec["nb_over_poisson_dense"] = rec["nb_dense_ms"] / rec["poisson_dense_ms"]
        rec["nb_sparse_ms"] = median_ms(lambda: ops.nb_deviance_sparse(*p, theta, s))
        rec["poisson_sparse_ms"] = median_ms(lambda: ops.poisson_deviance_sparse(*p, s))
        a, b = ops.nb_deviance(*p, theta, y), ops.nb_deviance_sparse(*p, theta, s)
        for k in ("total", "null_total", "loglik", "poisson_loglik"):
            rec[k + "_dense"], rec[k + "_sparse"] = float(a[k]), float(b[k])
        if density == 0.05:
            rec["torch_ms"], rec["torch_peak_MiB"] = torch_point(*p, theta, y)
            t = torch_composition(*p, theta, y)
            rec["total_torch"], rec["loglik_torch"] = float(t[0].sum()), float(t[3].sum())
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        del y, s
        torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
