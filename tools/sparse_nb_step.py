#!/usr/bin/env python3
"""Time the sparse negative-binomial step (ops.nb_nsf_sparse) next to the dense one (ops.nb_nsf) on the same counts in the
same process: median of 30 calls after warm-up, RUNS such medians per figure with the two forms alternating, synthetic
counts at 1 %, 5 % and 20 % density, at

  slideseq   N = 39 694 spots of which B = 7000 per step, D = 17 702, Lt = 20, E = 3   (the Slide-seq mini-batch)
  benchmark  N = 1037, D = 80, Lt = 4, E = 20                                           (the reference's benchmark)

Per point: the step in both forms; for the batch shape the batch selection in both forms (dense ``y[:, idx]``, the sparse
view) and step + selection as a training loop pays them; the zero part of the sparse step alone (the same call on a
SparseCounts without entries: its non-zero passes then find nothing to do) and the non-zero part as the difference; the
peak device memory of a step with the counts held in each form (torch's allocator, the other form's counts freed or
subtracted).  The line "5 % criterion" says whether sparse step + view lies below dense step + gather by more than the
spread of the runs.

    python tools/sparse_nb_step.py [shape ...] [--runs 3] [--json FILE] [--once SHAPE DENSITY]

``--once`` runs one sparse step at one point and nothing else (for a profiler)."""
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

SHAPES = {"slideseq": dict(N=39694, B=7000, D=17702, Lt=20, E=3), "benchmark": dict(N=1037, B=None, D=80, Lt=4, E=20)}
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


def peak_bytes(fn):
    torch.cuda.synchronize()
    gc.collect()                              # tensors of earlier points that only a reference cycle still holds
    torch.cuda.empty_cache()
    ops.release_workspaces()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


def point(name, density, runs, once=False):
    sh = SHAPES[name]
    N, D, Lt, E = sh["N"], sh["D"], sh["Lt"], sh["E"]
    B = sh["B"] or N
    dev = torch.device("cuda")
    gc.collect()
    torch.cuda.empty_cache()
    g = torch.Generator().manual_seed(1)
    mean = (0.3 * torch.randn(Lt, B, generator=g)).to(dev)
    scale = (0.2 + 0.3 * torch.rand(Lt, B, generator=g)).to(dev)
    eps = torch.randn(E, Lt, B, generator=g).to(dev)
    W = (torch.rand(D, Lt, generator=g) + 0.05).to(dev)
    V = (0.5 + torch.rand(B, generator=g)).to(dev)
    theta = torch.logspace(math.log10(0.3), math.log10(50.0), D).to(dev)
    y = synthetic_counts(D, N, density, dev, seed=int(1000 * density))
    s = SparseCounts(y)
    idx = torch.randperm(N, generator=g)[:B].to(dev) if sh["B"] else None
    view = s if idx is None else s[:, idx]
    par = (mean, scale, eps, W, V, theta)
    if once:
        out = ops.nb_nsf_sparse(*par, view)
        torch.cuda.synchronize()
        print(f"{name} density {density}: loglik {float(out[0]):.3f}")
        return None
    empty = SparseCounts(torch.sparse_coo_tensor(torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0), (D, N))).to(dev)
    empty_view = empty if idx is None else empty[:, idx]
    yb = y if idx is None else y[:, idx]
    rec = dict(shape=name, N=N, B=B, D=D, Lt=Lt, E=E, density=density, nnz=s.nnz, nnz_batch=view.nnz,
               y_dense_bytes=y.numel() * 4, y_sparse_bytes=sparse_bytes(s), runs=[])
    for _ in range(runs):                     # the forms alternate inside a run
        r = dict(dense_ms=median_ms(lambda: ops.nb_nsf(*par, yb)), sparse_ms=median_ms(lambda: ops.nb_nsf_sparse(*par, view)),
                 zero_part_ms=median_ms(lambda: ops.nb_nsf_sparse(*par, empty_view)))
        r["nonzero_part_ms"] = r["sparse_ms"] - r["zero_part_ms"]
        if idx is not None:
            r["dense_gather_ms"] = median_ms(lambda: y[:, idx])
            with ops.deferred_info():          # as in the training loops: the index check is read once, behind the block
                r["sparse_gather_ms"] = median_ms(lambda: s[:, idx])
                r["sparse_total_ms"] = median_ms(lambda: ops.nb_nsf_sparse(*par, s[:, idx]))
            r["dense_total_ms"] = median_ms(lambda: ops.nb_nsf(*par, y[:, idx]))
        rec["runs"].append(r)
    for k in rec["runs"][0]:
        vals = [r[k] for r in rec["runs"]]
        rec[k], rec[k + "_spread"] = statistics.median(vals), max(vals) - min(vals)
    a = ops.nb_nsf(*par, yb)
    b = ops.nb_nsf_sparse(*par, view)
    rec["loglik_dense"], rec["loglik_sparse"] = float(a[0]), float(b[0])
    rec["max_rel_grad_diff"] = max(float((u - v).abs().max() / u.abs().max()) for u, v in zip(a[1:], b[1:]))
    del a, b, yb
    # peak memory of one step with its batch selection, the counts held in one form: torch's allocator, the other form's
    # counts subtracted (dense) or freed (sparse)
    held = sparse_bytes(s) + sparse_bytes(empty)
    rec["peak_dense_bytes"] = peak_bytes(lambda: ops.nb_nsf(*par, y if idx is None else y[:, idx])) - held
    del y
    with ops.deferred_info():
        rec["peak_sparse_bytes"] = peak_bytes(lambda: ops.nb_nsf_sparse(*par, s if idx is None else s[:, idx])) - sparse_bytes(empty)
    return rec


def main():
    args = sys.argv[1:]
    if "--once" in args:
        i = args.index("--once")
        point(args[i + 1], float(args[i + 2]), 1, once=True)
        return
    out, runs = None, 3
    if "--json" in args:
        i = args.index("--json")
        out = args[i + 1]
        del args[i:i + 2]
    if "--runs" in args:
        i = args.index("--runs")
        runs = int(args[i + 1])
        del args[i:i + 2]
    rows = []
    for name in (args or list(SHAPES)):
        for density in DENSITIES:
            r = point(name, density, runs)
            rows.append(r)
            print(f"{name:9s} density {density:4.2f}  nnz(batch) {r['nnz_batch']:>10d}  dense {r['dense_ms']:7.3f} ms (+-{r['dense_ms_spread']:.3f})  "
                  f"sparse {r['sparse_ms']:7.3f} ms (+-{r['sparse_ms_spread']:.3f})  = zero part {r['zero_part_ms']:.3f} + non-zero part "
                  f"{r['nonzero_part_ms']:.3f}  rel grad diff {r['max_rel_grad_diff']:.1e}", flush=True)
            print(f"          counts {r['y_dense_bytes'] / 2 ** 20:8.1f} MiB dense, {r['y_sparse_bytes'] / 2 ** 20:7.1f} MiB sparse; peak of a step "
                  f"{r['peak_dense_bytes'] / 2 ** 20:8.1f} MiB dense, {r['peak_sparse_bytes'] / 2 ** 20:7.1f} MiB sparse", flush=True)
            if "dense_gather_ms" in r:
                print(f"          y[:, idx] dense {r['dense_gather_ms']:.3f} ms, sparse view {r['sparse_gather_ms']:.3f} ms; step + selection "
                      f"dense {r['dense_total_ms']:.3f} ms (+-{r['dense_total_ms_spread']:.3f}), sparse {r['sparse_total_ms']:.3f} ms "
                      f"(+-{r['sparse_total_ms_spread']:.3f})", flush=True)
                if abs(density - 0.05) < 1e-9:
                    gain = r["dense_total_ms"] - r["sparse_total_ms"]
                    spread = max(r["dense_total_ms_spread"], r["sparse_total_ms_spread"])
                    print(f"          5 % criterion: sparse step + view lower by {gain:.3f} ms, spread of the runs {spread:.3f} ms: "
                          f"{'met' if gain > spread else 'NOT met'}", flush=True)
            torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
