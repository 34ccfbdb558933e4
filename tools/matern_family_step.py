#!/usr/bin/env python3
"""Time the fused forward and forward + backward for the three Matern smoothness values, and print one JSON line.

    python tools/matern_family_step.py [--shapes 200000x2048x32,50000x512x8] [--kinds matern12,matern32,matern52]
                                       [--reps 7] [--warmup 2] [--paths]

Per shape (N x M x L, fp32, whitened, the draws of BASELINE config 3 under each kernel) and kind, in ONE process, HIP-event
times of `reps` calls after `warmup` calls:
  `forward_ms`          one ELBO evaluation (ops.svgp_forward with y: the headline workload of bench.py)
  `train_mu_Lu_ms`      forward + backward to mu and Lu, as bench.py's training leg runs it (factor handed over, Wt retained)
  `train_all_ms`        ... to mu, Lu, Z, sigma and lengthscale (the kernel gradients: csrc/kgrad.hip)
each as the median, with `_min` / `_max` over the calls, `path` (gpz_svgp_forward_path: bit 0 wide tiles, bit 1 generated
operand, 4 panel kernel) and `vs_matern32` = median / Matern-3/2's median at the same shape in the same run.  The kinds are
measured round-robin, call by call, so a drift of the engine clock lands on all three alike.
--paths: also `forward_generated_ms` (materialize_kzx=False: stage 1 generates its covariance operand) and, for M <= 512,
`forward_tiles_ms` (materialize_kzx=True: the fill + tile kernels instead of the panel kernel)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd.configs import spec_for_config  # noqa: E402
from gpzoo_amd.synthetic import make_config  # noqa: E402


def problem(kind, N, M, L, dev):
    c = make_config(3, N=N, M=M, L=L, **({} if kind == "matern32" else {"kind": kind}))
    g = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    spec, extra = spec_for_config(g)
    return c, g, spec, extra


def forward(p, **kw):
    c, g, spec, extra = p
    return ops.svgp_forward(spec, g["X"], g["Z"], g["mu"], g["Lu_raw"], c["jitter"], c["whitened"], y=g["y"],
                            noise_sd=c["noise_sd"], want_Lu=False, **extra, **kw)


def train(p, kernel_grads):
    c, g, spec, extra = p
    handoff = ops.FactorCache()
    with ops.deferred_info():
        o = ops.svgp_forward(spec, g["X"], g["Z"], g["mu"], g["Lu_raw"], c["jitter"], c["whitened"], want_Lu=False,
                             retain_wt=1.0 / 3, cache=handoff, **extra)
        gmean = (o["mean"] - g["y"]) / c["noise_sd"] ** 2
        gscale = o["scale"] / c["noise_sd"] ** 2
        return ops.svgp_backward(spec, g["X"], g["Z"], g["mu"], g["Lu_raw"], c["jitter"], c["whitened"], gmean, gscale,
                                 o["scale"], kernel_grads=kernel_grads, wt_cache=o.pop("wt_cache", None), cache=handoff,
                                 trust_cache=True, trust_qu=True, **extra)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(N, M, L, kinds, args, dev):
    probs = {k: problem(k, N, M, L, dev) for k in kinds}
    legs = {"forward": lambda p: forward(p), "train_mu_Lu": lambda p: train(p, False), "train_all": lambda p: train(p, True)}
    if args.paths:
        legs["forward_generated"] = lambda p: forward(p, materialize_kzx=False)
        if M <= 512:
            legs["forward_tiles"] = lambda p: forward(p, materialize_kzx=True)
    out = {k: {"path": int(forward(probs[k])["path"])} for k in kinds}
    for leg, fn in legs.items():
        ms = {k: [] for k in kinds}
        for i in range(args.warmup + args.reps):
            for k in kinds:                       # round-robin: every kind sees the same clock
                t = timed(lambda: fn(probs[k]))
                if i >= args.warmup:
                    ms[k].append(t)
        torch.cuda.empty_cache()
        for k in kinds:
            v = sorted(ms[k])
            out[k].update({f"{leg}_ms": v[len(v) // 2], f"{leg}_ms_min": v[0], f"{leg}_ms_max": v[-1]})
        if "matern32" in kinds:
            for k in kinds:
                out[k][f"{leg}_vs_matern32"] = out[k][f"{leg}_ms"] / out["matern32"][f"{leg}_ms"]
    return {k: {n: (float(f"{v:.5g}") if isinstance(v, float) else v) for n, v in r.items()} for k, r in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200000x2048x32,50000x512x8")
    ap.add_argument("--kinds", default="matern12,matern32,matern52")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--paths", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    kinds = [k for k in args.kinds.split(",") if k]
    out = {"tool": "matern_family_step", "reps": args.reps, "warmup": args.warmup, "dtype": "fp32", "shapes": {}}
    for s in args.shapes.split(","):
        N, M, L = (int(v) for v in s.split("x"))
        out["shapes"][s] = measure(N, M, L, kinds, args, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
