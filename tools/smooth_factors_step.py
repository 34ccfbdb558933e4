#!/usr/bin/env python3
"""Time smooth_spatial_factors -- the exact K-nearest mean (gpz_knn_mean) and the whole public call -- and print one
JSON line.

    python tools/smooth_factors_step.py [--shapes 1037x100x4,40000x3000x20,200000x2048x32] [--reps 20] [--threads 16]

Per shape (N spots, M inducing points, L factors; d = 2, float32, K = max(2, ceil(N / M)); spots on a uniform disc plus
dense clusters, inducing points = a random subset of the spots): after a warm-up, `reps` calls timed one by one --
`knn_ms` the library call alone (HIP events), `public_ms` gpzoo.utilities.smooth_spatial_factors on numpy inputs (host
clock around the call, which ends in device-to-host copies: uploads, the finiteness check, the selection, the trend) --
each as median, min and max.  `passes`: the mean number of sweeps over the spots per query (radix-select passes + the
gather sweep), counted on the host for 64 sampled queries from the same keys; `gpairs_per_s` = M N passes / knn median.
With sklearn importable the same step composed as the reference does (LinearRegression + KNeighborsRegressor, n_jobs =
`threads`) is timed next to it (`sklearn_ms`: median, min, max of 3) and the largest difference of U is reported."""
import argparse
import json
import os
import sys
import time
from math import ceil

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import _lib, ops  # noqa: E402
from gpzoo_amd.utilities import smooth_spatial_factors  # noqa: E402


def points(N, seed=0):
    rng = np.random.default_rng(seed)
    n_disc = N * 3 // 4
    r, t = np.sqrt(rng.random(n_disc)) * 100.0, rng.random(n_disc) * 2 * np.pi
    disc = np.stack([r * np.cos(t), r * np.sin(t)], 1)
    centres = rng.random((25, 2)) * 160.0 - 80.0
    clusters = centres[rng.integers(0, 25, N - n_disc)] + rng.normal(size=(N - n_disc, 2)) * 0.05
    return np.concatenate([disc, clusters])[rng.permutation(N)].astype(np.float32)


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}


def sweeps(X, Z, K, rows):
    """Mean sweeps per query of gpz_knn_mean (csrc/smooth.hip): digits of 11, 8 x 6 and 4 bits from the top of d^2's bit
    pattern until every key that shares the K-th key's decided bits is selected, plus the gather sweep."""
    X, Z = X.astype(np.float64), Z.astype(np.float64)
    total = 0
    for m in rows:
        d2 = (X[:, 0] - Z[m, 0]) ** 2
        for k in range(1, X.shape[1]):
            d2 = d2 + (X[:, k] - Z[m, k]) ** 2
        key = np.sort(d2).view(np.uint64)
        for n_pass, low in enumerate((52, 44, 36, 28, 20, 12, 4, 0), start=1):
            hi = key >> np.uint64(low)
            below, members = int((hi < hi[K - 1]).sum()), int((hi == hi[K - 1]).sum())
            if members == K - below or low == 0:
                break
        total += n_pass + 1
    return total / len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1037x100x4,40000x3000x20,200000x2048x32")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda")
    s = ops._stream(dev)
    out = {"tool": "smooth_factors_step", "d": 2, "dtype": "float32", "reps": args.reps, "shapes": {}}
    for shape in args.shapes.split(","):
        N, M, L = (int(v) for v in shape.split("x"))
        K = max(2, ceil(N / M))
        rng = np.random.default_rng(N)
        Xh = points(N)
        Zh = Xh[rng.choice(N, M, replace=False)]
        Fh = (np.sin(Xh[:, :1] * rng.random(L)) + 0.3 * rng.normal(size=(N, L)) - 1.5).astype(np.float32)
        X, Z, F = (torch.as_tensor(a, device=dev) for a in (Xh, Zh, Fh))
        U = torch.empty((M, L), dtype=torch.float64, device=dev)
        ws = torch.empty(lib.gpz_knn_mean_workspace_bytes(N, M, 2, K, L), dtype=torch.uint8, device=dev)

        def knn():
            _lib.check(lib.gpz_knn_mean(ops._ptr(X), N, ops._ptr(Z), M, 2, _lib.GPZ_F32, ops._ptr(F), L, _lib.GPZ_F32, K,
                                        ops._ptr(U), None, ops._ptr(ws), ws.numel(), s), "gpz_knn_mean")

        for _ in range(3):
            knn()
            smooth_spatial_factors(Fh, Zh, Xh)
        torch.cuda.synchronize()
        knn_ms, public_ms = [], []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            knn()
            b.record()
            b.synchronize()
            knn_ms.append(a.elapsed_time(b))
        for _ in range(args.reps):
            t0 = time.perf_counter()
            got = smooth_spatial_factors(Fh, Zh, Xh)
            public_ms.append((time.perf_counter() - t0) * 1e3)
        passes = sweeps(Xh, Zh, K, rng.choice(M, min(M, 64), replace=False))
        r = {"K": K, "knn_ms": stats(knn_ms), "public_ms": stats(public_ms), "passes": round(passes, 3),
             "gpairs_per_s": round(M * N * passes / (float(np.median(knn_ms)) * 1e-3) / 1e9, 2)}
        try:
            from sklearn.linear_model import LinearRegression
            from sklearn.neighbors import KNeighborsRegressor
        except ImportError:
            LinearRegression = None
        if LinearRegression is not None:
            sk_ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                lr = LinearRegression(n_jobs=args.threads).fit(Xh, Fh)
                Us = KNeighborsRegressor(n_neighbors=K, n_jobs=args.threads).fit(Xh, Fh).predict(Zh)
                sk_ms.append((time.perf_counter() - t0) * 1e3)
            r["sklearn_ms"] = stats(sk_ms)
            r["sklearn_threads"] = args.threads
            r["U_max_abs_diff_sklearn"] = float(np.abs(Us - got[0]).max())
            r["beta_max_abs_diff_sklearn"] = float(np.abs(lr.coef_ - got[2]).max())
        out["shapes"][shape] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
