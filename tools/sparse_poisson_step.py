#!/usr/bin/env python3
"""Time the sparse Poisson step (ops.poisson_nsf_sparse) next to the dense one (ops.poisson_nsf) on the same inputs in the
same process: median of 30 calls after warm-up, synthetic counts at 1 %, 5 % and 20 % density, at

  slideseq   N = 39 694 spots of which N_b = 7000 per step, D = 17 702, Lt = 20, E = 3   (the Slide-seq mini-batch)
  full       N = 39 694, D = 2000, Lt = 20, E = 3                                        (full batch)
  benchmark  N = 1037, D = 80, Lt = 4, E = 20                                            (the reference's benchmark)

Also reported: the bytes held for y in each form and, for the batch shape, the time of y[:, idx] itself in both forms.

    python tools/sparse_poisson_step.py [shape ...] [--json FILE] [--once SHAPE DENSITY]

``--once`` runs one sparse step at one point and nothing else (for a profiler)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd.likelihoods import SparseCounts  # noqa: E402

SHAPES = {"slideseq": dict(N=39694, B=7000, D=17702, Lt=20, E=3), "full": dict(N=39694, B=None, D=2000, Lt=20, E=3),
          "benchmark": dict(N=1037, B=None, D=80, Lt=4, E=20)}
DENSITIES = (0.01, 0.05, 0.20)
REPS, WARM = 30, 5


def median_ms(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def synthetic_counts(D, N, density, dev, seed):
    """(D, N) fp32 counts on the device: Poisson(2) + 1 where a uniform draw falls below ``density``, built in column
    blocks so that no temporary is larger than the result."""
    g = torch.Generator(device=dev).manual_seed(seed)
    y = torch.empty((D, N), dtype=torch.float32, device=dev)
    for n0 in range(0, N, 4096):
        n1 = min(N, n0 + 4096)
        keep = torch.rand((D, n1 - n0), generator=g, device=dev) < density
        y[:, n0:n1] = (torch.poisson(torch.full((D, n1 - n0), 2.0, device=dev), generator=g) + 1.0) * keep
    return y


def sparse_bytes(s):
    return sum(getattr(s, k).numel() * getattr(s, k).element_size() for k in s._PARTS)


def point(name, density, once=False):
    sh = SHAPES[name]
    N, D, Lt, E = sh["N"], sh["D"], sh["Lt"], sh["E"]
    B = sh["B"] or N
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1)
    mean = (0.3 * torch.randn(Lt, B, generator=g)).to(dev)
    scale = (0.2 + 0.3 * torch.rand(Lt, B, generator=g)).to(dev)
    eps = torch.randn(E, Lt, B, generator=g).to(dev)
    W = (torch.rand(D, Lt, generator=g) + 0.05).to(dev)
    V = (0.5 + torch.rand(B, generator=g)).to(dev)
    y = synthetic_counts(D, N, density, dev, seed=int(1000 * density))
    s = SparseCounts(y)
    idx = torch.randperm(N, generator=g)[:B].to(dev) if sh["B"] else None
    view = s if idx is None else s[:, idx]
    if once:
        out = ops.poisson_nsf_sparse(mean, scale, eps, W, V, view)
        torch.cuda.synchronize()
        print(f"{name} density {density}: loglik {float(out[0]):.3f}")
        return None
    yb = y if idx is None else y[:, idx]
    rec = dict(shape=name, N=N, B=B, D=D, Lt=Lt, E=E, density=density, nnz=s.nnz, nnz_batch=view.nnz,
               y_dense_bytes=y.numel() * 4, y_sparse_bytes=sparse_bytes(s))
    rec["dense_ms"] = median_ms(lambda: ops.poisson_nsf(mean, scale, eps, W, V, yb))
    rec["sparse_ms"] = median_ms(lambda: ops.poisson_nsf_sparse(mean, scale, eps, W, V, view))
    if idx is not None:
        rec["dense_gather_ms"] = median_ms(lambda: y[:, idx])
        with ops.deferred_info():          # as in the training loops: the index check is read once, behind the block
            rec["sparse_gather_ms"] = median_ms(lambda: s[:, idx])
    a = ops.poisson_nsf(mean, scale, eps, W, V, yb)
    b = ops.poisson_nsf_sparse(mean, scale, eps, W, V, view)
    rec["loglik_dense"], rec["loglik_sparse"] = float(a[0]), float(b[0])
    rec["max_rel_grad_diff"] = max(float((u - v).abs().max() / u.abs().max()) for u, v in zip(a[1:], b[1:]))
    return rec


def main():
    args = sys.argv[1:]
    if "--once" in args:
        i = args.index("--once")
        point(args[i + 1], float(args[i + 2]), once=True)
        return
    out = None
    if "--json" in args:
        i = args.index("--json")
        out = args[i + 1]
        del args[i:i + 2]
    rows = []
    for name in (args or list(SHAPES)):
        for density in DENSITIES:
            r = point(name, density)
            rows.append(r)
            gather = (f"  y[:, idx] dense {r['dense_gather_ms']:.3f} ms, sparse {r['sparse_gather_ms']:.3f} ms"
                      if "dense_gather_ms" in r else "")
            print(f"{name:9s} density {density:4.2f}  nnz(batch) {r['nnz_batch']:>10d}  dense {r['dense_ms']:7.3f} ms  sparse "
                  f"{r['sparse_ms']:7.3f} ms  ({r['dense_ms'] / r['sparse_ms']:5.2f}x)  y {r['y_dense_bytes'] / 2 ** 20:8.1f} MiB dense, "
                  f"{r['y_sparse_bytes'] / 2 ** 20:7.1f} MiB sparse{gather}  rel grad diff {r['max_rel_grad_diff']:.1e}", flush=True)
            torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
