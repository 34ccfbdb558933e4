#!/usr/bin/env python3
"""Time project_factors_to_inducing -- the Gram pass alone (gpz_kernel_gram) and the whole public call -- and print one
JSON line.

    python tools/projection_step.py [--shapes notebook,config3,hybrid32,hybrid64] [--reps 20]

Shapes: `notebook` N = 39 694, M = 3 000, L = 10, RBF (NSF_RBF), fp32; `config3` N = 200 000, M = 2 048, L = 32, Matern-3/2
per latent, fp32; `hybrid32` / `hybrid64` N = 1 037, M = 529, L = 4, RBF per latent, fp32 / fp64.  d = 2; inputs by the
tests' recipe (inducing points on a displaced grid, lengthscale half its pitch).

Per shape, after two warm-up calls, `reps` calls timed one by one, each ending in a device synchronise (HIP events), as
median / min / max in ms: `gram_ms` ops.kernel_gram alone, `public_ms` project_factors_to_inducing on CUDA tensors (host
clock).  `gram_tflops`: the lower-triangle count L M (M + 128) N over the Gram pass's median.  `gram_workspace_mb`:
gpz_kernel_gram_workspace_bytes; `public_peak_mb`: torch's peak allocation during one call over what was allocated before
it; `kzx_mb`: what a stored K_zx would take.  The notebooks' own composition on torch (bmm, torch.linalg.cholesky,
torch.cholesky_solve) is not timed here: it ended in a HIP launch failure on the MI355X at every shape when it was tried,
the cause is not known, and it stays out until it is."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpzoo_amd import kernels as K, ops  # noqa: E402
from gpzoo_amd.utilities import project_factors_to_inducing  # noqa: E402
import projection_cases as PC  # noqa: E402

SHAPES = {"notebook": (39694, 3000, 10, "NSF_RBF", torch.float32), "config3": (200000, 2048, 32, "batched_Matern32", torch.float32),
          "hybrid32": (1037, 529, 4, "NSF_RBF", torch.float32), "hybrid64": (1037, 529, 4, "NSF_RBF", torch.float64)}
JITTER = 1e-5


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}


def timed(fn, reps, host_clock=False):
    ms = []
    for _ in range(reps):
        if host_clock:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
    return ms


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="notebook,config3,hybrid32,hybrid64")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = {"tool": "projection_step", "d": 2, "reps": args.reps, "jitter": JITTER, "shapes": {}}
    for name in args.shapes.split(","):
        N, M, L, cls, dt = SHAPES[name]
        inp = PC.recipe(N, M, L, 0.5, 0, per_latent=True)
        if cls == "NSF_RBF":
            kernel = K.NSF_RBF(L=L)
            kernel.sigma.data = torch.as_tensor(inp["sigma"]).reshape(L, 1, 1).to(dt)
            kernel.lengthscale.data = torch.as_tensor(inp["lengthscale"]).reshape(L, 1, 1).to(dt)
        else:
            kernel = getattr(K, cls)()
            kernel.sigma.data, kernel.lengthscale.data = torch.as_tensor(inp["sigma"]).to(dt), torch.as_tensor(inp["lengthscale"]).to(dt)
        kernel = kernel.to(dev)
        Z, X, F = (torch.as_tensor(inp[k]).to(device=dev, dtype=dt) for k in ("Z", "X", "F"))
        spec = K.kernel_spec(kernel, X)
        plan = ops.kernel_gram_plan(N, M, L, dt)
        r = {"N": N, "M": M, "L": L, "kernel": cls, "dtype": str(dt).replace("torch.", ""), "n_splits": plan["n_splits"],
             "cols_per_split": plan["cols_per_split"], "gram_workspace_mb": round(plan["workspace_bytes"](1) / 2 ** 20, 1)}

        def gram():
            return ops.kernel_gram(spec, Z, X, F, JITTER)

        def public():
            return project_factors_to_inducing(kernel, Z, X, F, jitter=JITTER)

        for _ in range(2):
            gram()
            public()
        torch.cuda.synchronize()
        gram_ms = timed(gram, args.reps)
        r["gram_ms"] = stats(gram_ms)
        r["gram_tflops"] = round(L * M * (M + 128) * N / (float(np.median(gram_ms)) * 1e-3) / 1e12, 2)
        r["public_ms"] = stats(timed(public, args.reps, host_clock=True))
        r["public_peak_mb"] = peak_mb(public)
        r["kzx_mb"] = round(L * M * N * (4 if dt == torch.float32 else 8) / 2 ** 20, 1)
        out["shapes"][name] = r
        print(json.dumps({name: r}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
