#!/usr/bin/env python3
"""Time kmeans_inducing_points -- the k-means++ seeding (gpz_kmeans_seed), one Lloyd iteration (gpz_kmeans_lloyd) and the
whole public call -- and print one JSON line.

    python tools/kmeans_step.py [--shapes 39694x3000,200000x2048,7000x3000] [--reps 10] [--threads 16] [--no-sklearn]

Per shape (N spots, M centres; d = 2, float32; spots on a uniform disc plus dense clusters): after a warm-up, `seed_ms`
the seeding alone and `lloyd_iter_ms` one iteration from the seeded centres (HIP events around the library call, `reps`
calls timed one by one), `public_ms` gpzoo.utilities.kmeans_inducing_points on numpy input (host clock around the call:
upload, finiteness check, seeding, every iteration with one read of the stop record per 16, final labels and inertia,
download; 3 calls) -- each as median, min and max -- with `n_iter`, `converged` and `inertia` of that call.
`gdist_per_s`: N M distances per iteration over the iteration's median.  With sklearn importable (and no --no-sklearn)
``KMeans(n_clusters=M, n_init=1, algorithm="lloyd", random_state=0)`` on `threads` host threads is timed next to it
(`sklearn_ms`, one call) with its n_iter_ and inertia_; its draws differ, so the two runs are two samples of one method."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd.utilities import kmeans_inducing_points  # noqa: E402


def points(N, seed=0):
    rng = np.random.default_rng(seed)
    n_disc = N * 3 // 4
    r, t = np.sqrt(rng.random(n_disc)) * 100.0, rng.random(n_disc) * 2 * np.pi
    disc = np.stack([r * np.cos(t), r * np.sin(t)], 1)
    centres = rng.random((25, 2)) * 160.0 - 80.0
    clusters = centres[rng.integers(0, 25, N - n_disc)] + rng.normal(size=(N - n_disc, 2)) * 0.5
    return np.concatenate([disc, clusters])[rng.permutation(N)].astype(np.float32)


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="39694x3000,200000x2048,7000x3000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = {"tool": "kmeans_step", "d": 2, "dtype": "float32", "reps": args.reps, "shapes": {}}
    for shape in args.shapes.split(","):
        N, M = (int(v) for v in shape.split("x"))
        Xh = points(N)
        X = torch.as_tensor(Xh, device=dev)
        T = 2 + int(np.log(M))
        u = torch.as_tensor(np.random.default_rng(0).random((M, T)), device=dev)
        _, C0 = ops.kmeans_seed(X, M, u)
        labels = torch.full((N,), -1, dtype=torch.int32, device=dev)

        def one_iteration():
            ops.kmeans_lloyd(X, C0.clone(), labels, ops.kmeans_state(dev), 0.0, 1)

        for _ in range(2):
            one_iteration()
        torch.cuda.synchronize()
        seed_ms = timed(lambda: ops.kmeans_seed(X, M, u), max(3, args.reps // 3))
        iter_ms = timed(one_iteration, args.reps)
        public_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            _, info = kmeans_inducing_points(Xh, M, random_state=0, return_info=True)
            public_ms.append((time.perf_counter() - t0) * 1e3)
        r = {"seed_ms": stats(seed_ms), "lloyd_iter_ms": stats(iter_ms), "public_ms": stats(public_ms), "n_iter": info["n_iter"],
             "converged": info["converged"], "inertia": info["inertia"],
             "gdist_per_s": round(N * M / (float(np.median(iter_ms)) * 1e-3) / 1e9, 2)}
        KMeans = None
        if not args.no_sklearn:
            try:
                from sklearn.cluster import KMeans
            except ImportError:
                pass
        if KMeans is not None:
            import contextlib
            try:
                from threadpoolctl import threadpool_limits
                limit = threadpool_limits(limits=args.threads)
            except ImportError:
                limit = contextlib.nullcontext()
            with limit:
                t0 = time.perf_counter()
                km = KMeans(n_clusters=M, n_init=1, algorithm="lloyd", random_state=0).fit(Xh)
                r["sklearn_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            r.update(sklearn_threads=args.threads, sklearn_n_iter=int(km.n_iter_), sklearn_inertia=float(km.inertia_))
        out["shapes"][shape] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
