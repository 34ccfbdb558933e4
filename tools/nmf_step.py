#!/usr/bin/env python3
"""Time the fused KL multiplicative-update NMF (gpz_nmf_kl_update) on planted count matrices, and print one JSON line.

    python tools/nmf_step.py [--shapes 1037x80x4,40000x2000x20,200000x2000x32] [--f64 40000x2000x20]
                             [--iters 20] [--reps 7] [--no-torch] [--sklearn] [--end-to-end 40000x2000x20]

Per shape and dtype, HIP-event times of `reps` calls of `iters` iterations each after a warm-up call:
`iter_ms` (median per iteration), `iter_ms_min` / `iter_ms_max` (the spread over the calls), the achieved `GB_per_s`
against the 2 N D sizeof(T) bytes of X an iteration has to read and `TFLOP_per_s` against its 8 N D Lp flops (Lp = L
padded to the k-steps the kernel runs), the two floors `hbm_floor_ms` (6.3 TB/s, the measured copy rate) and
`mfma_floor_ms` (155 TFLOP/s fp32, 78 fp64), and `of_floor` = the larger floor / iter_ms.  `divergence_ms`: one
gpz_nmf_kl_divergence with its scalar read-back.
Baselines, neither of them the library: `torch_iter_ms`, the same iteration composed from torch.matmul and element-wise
operations on the same GPU (it materialises P and Q), with `torch_max_rel_diff` of its W against the library's after
`iters` iterations; with --sklearn, `sklearn_iter_ms` of sklearn's _fit_multiplicative_update on this host's CPU.
--end-to-end: wall time of regularized_nmf (nndsvdar, tol = 0) for max_iter = 20 and 1000 and of its initialisation."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import _lib, nmf, ops  # noqa: E402

EPS = float(np.finfo(np.float32).eps)
KSTEPS = (1, 2, 3, 4, 5, 8, 12, 16)


def planted(N, D, L, dtype, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    F = torch._standard_gamma(torch.full((N, L), 0.6, device=dev), generator=g)
    W = torch._standard_gamma(torch.full((L, D), 0.5, device=dev), generator=g)
    X = torch.poisson(6.0 * (F @ W) / L, generator=g).to(dtype)
    W0 = torch.rand(N, L, device=dev, generator=g).to(dtype) + 0.1
    H0 = torch.rand(L, D, device=dev, generator=g).to(dtype) + 0.1
    return X, W0, H0


def torch_iteration(X, W, H):
    P = (W @ H).clamp_(min=EPS)
    den = H.sum(1)
    den[den == 0] = EPS
    W = W * ((X / P) @ H.T / den)
    P = (W @ H).clamp_(min=EPS)
    ws = W.sum(0)
    ws[ws == 0] = 1.0
    H = H * (W.T @ (X / P) / ws[:, None])
    H[H < np.finfo(np.float64).eps] = 0
    return W, H


def timed_calls(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def measure(N, D, L, dtype, args, lib, dev):
    X, W0, H0 = planted(N, D, L, dtype, dev)
    size = X.element_size()
    code = _lib.GPZ_F32 if dtype == torch.float32 else _lib.GPZ_F64
    ws = torch.empty(lib.gpz_nmf_kl_workspace_bytes(N, D, L, code), dtype=torch.uint8, device=dev)
    s = ops._stream(dev)
    W, H = W0.clone(), H0.clone()

    def update():
        _lib.check(lib.gpz_nmf_kl_update(ops._ptr(X), ops._ptr(W), ops._ptr(H), N, D, L, code, args.iters, ops._ptr(ws),
                                         ws.numel(), s), "gpz_nmf_kl_update")

    ms = sorted(t / args.iters for t in timed_calls(update, args.reps))
    it = ms[len(ms) // 2]
    Lp = 4 * next(k for k in KSTEPS if 4 * k >= L)
    traffic, flops = 2.0 * N * D * size, 8.0 * N * D * Lp
    hbm, mfma = traffic / 6.3e12 * 1e3, flops / (155e12 if dtype == torch.float32 else 78e12) * 1e3
    r = {"iter_ms": it, "iter_ms_min": ms[0], "iter_ms_max": ms[-1], "GB_per_s": traffic / it / 1e6,
         "TFLOP_per_s": flops / it / 1e9, "hbm_floor_ms": hbm, "mfma_floor_ms": mfma, "of_floor": max(hbm, mfma) / it,
         "workspace_MB": ws.numel() / 1e6}
    t0 = time.perf_counter()
    ops.nmf_kl_divergence(X, W, H)
    r["divergence_ms"] = (time.perf_counter() - t0) * 1e3
    Wl, _, _ = ops.nmf_kl_mu(X, W0, H0, max_iter=args.iters, tol=0)
    if not args.no_torch:
        state = [W0, H0]

        def torch_run():
            w, h = W0, H0
            for _ in range(args.iters):
                w, h = torch_iteration(X, w, h)
            state[0], state[1] = w, h

        tm = sorted(t / args.iters for t in timed_calls(torch_run, max(3, args.reps // 2)))
        r["torch_iter_ms"] = tm[len(tm) // 2]
        r["torch_over_fused"] = r["torch_iter_ms"] / it
        r["torch_max_rel_diff"] = float((state[0] - Wl).abs().max() / Wl.abs().max())
    if args.sklearn:
        from sklearn.decomposition._nmf import _fit_multiplicative_update
        Xh, Wh, Hh = X.cpu().numpy(), W0.cpu().numpy().copy(), H0.cpu().numpy().copy()
        k = 3 if N * D > 5e7 else 10
        t0 = time.perf_counter()
        _fit_multiplicative_update(Xh, Wh, Hh, "kullback-leibler", max_iter=k, tol=0)
        r["sklearn_iter_ms"] = (time.perf_counter() - t0) * 1e3 / k
        r["sklearn_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
    return {k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in r.items()}


def end_to_end(N, D, L, dev):
    from gpzoo_amd.utilities import regularized_nmf
    Y, _, _ = planted(N, D, L, torch.float32, dev, seed=1)
    kw = dict(solver="mu", beta_loss="kullback-leibler", init="nndsvdar", tol=0.0, random_state=997, shrinkage=0.3)
    regularized_nmf(Y, L, max_iter=2, **kw)                   # warm-up
    r = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nmf.initialize_nmf(Y, L, init="nndsvdar", random_state=997)
    torch.cuda.synchronize()
    r["init_ms"] = (time.perf_counter() - t0) * 1e3
    for k in (20, 1000):
        t0 = time.perf_counter()
        regularized_nmf(Y, L, max_iter=k, **kw)
        r[f"max_iter_{k}_ms"] = (time.perf_counter() - t0) * 1e3
        r[f"max_iter_{k}_init_share"] = r["init_ms"] / r[f"max_iter_{k}_ms"]
    return {k: float(f"{v:.4g}") for k, v in r.items()}


def shapes(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1037x80x4,40000x2000x20,200000x2000x32")
    ap.add_argument("--f64", default="40000x2000x20")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--end-to-end", default="")
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda")
    out = {"tool": "nmf_step", "iters_per_call": args.iters, "reps": args.reps, "fp32": {}, "fp64": {}}
    for N, D, L in shapes(args.shapes):
        out["fp32"][f"{N}x{D}x{L}"] = measure(N, D, L, torch.float32, args, lib, dev)
    for N, D, L in shapes(args.f64):
        out["fp64"][f"{N}x{D}x{L}"] = measure(N, D, L, torch.float64, args, lib, dev)
    for N, D, L in shapes(args.end_to_end):
        out.setdefault("end_to_end", {})[f"{N}x{D}x{L}"] = end_to_end(N, D, L, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
