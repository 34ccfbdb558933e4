#!/usr/bin/env python3
"""Time dims_autocorr's two GPU stages -- the self-kNN graph (gpz_spatial_knn) and Moran's I (gpz_morans_i) -- on a
uniform disc plus dense clusters (d = 2, K = 6; L = 32 factors), and print one JSON line.

    python tools/spatial_autocorr_step.py [--sizes 200000,1000000] [--reps 20]

Per size: `order_ms` (ops.morton_order, the search order), `knn_ms` (the library call alone, given the order),
`graph_ms` (ops.spatial_knn: both), `moran_ms` (the library call alone), `moran_checked_ms` (ops.morans_i: with the
read-back of its info word) -- HIP-event means over `reps` calls after a warm-up.  With sklearn importable, also the
CPU time of NearestNeighbors(6).kneighbors() plus a numpy Moran's I on the same inputs, for context."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import _lib, ops  # noqa: E402


def points(N, seed=0):
    rng = np.random.default_rng(seed)
    n_disc = N * 3 // 4
    r, t = np.sqrt(rng.random(n_disc)) * 100.0, rng.random(n_disc) * 2 * np.pi
    disc = np.stack([r * np.cos(t), r * np.sin(t)], 1)
    centres = rng.random((25, 2)) * 160.0 - 80.0
    clusters = centres[rng.integers(0, 25, N - n_disc)] + rng.normal(size=(N - n_disc, 2)) * 0.05
    return np.concatenate([disc, clusters])[rng.permutation(N)].astype(np.float32)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200000,1000000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--L", type=int, default=32)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda")
    s = ops._stream(dev)
    out = {"tool": "spatial_autocorr_step", "d": 2, "K": 6, "L": args.L, "sizes": {}}
    for N in [int(v) for v in args.sizes.split(",")]:
        Xh = points(N)
        X = torch.as_tensor(Xh, device=dev)
        K, L = 6, args.L
        F = torch.rand(N, L, device=dev) + torch.sin(X[:, :1] * torch.rand(L, device=dev))
        order = ops.morton_order(X)
        idx = torch.empty((N, K), dtype=torch.int64, device=dev)
        ws = torch.empty(lib.gpz_spatial_knn_workspace_bytes(N, 2, K), dtype=torch.uint8, device=dev)

        def knn():
            _lib.check(lib.gpz_spatial_knn(ops._ptr(X), N, 2, K, _lib.GPZ_F32, ops._ptr(order), ops._ptr(idx),
                                           ops._ptr(ws), ws.numel(), s), "gpz_spatial_knn")

        I = torch.empty(L, dtype=torch.float64, device=dev)
        info = torch.empty(1, dtype=torch.int32, device=dev)
        wm = torch.empty(lib.gpz_morans_i_workspace_bytes(N, L, K), dtype=torch.uint8, device=dev)

        def moran():
            _lib.check(lib.gpz_morans_i(ops._ptr(F), N, L, _lib.GPZ_F32, ops._ptr(idx), K, ops._ptr(I), ops._ptr(info),
                                        ops._ptr(wm), wm.numel(), s), "gpz_morans_i")

        r = {"order_ms": timed(lambda: ops.morton_order(X), args.reps), "knn_ms": timed(knn, args.reps),
             "graph_ms": timed(lambda: ops.spatial_knn(X, K), args.reps), "moran_ms": timed(moran, args.reps),
             "moran_checked_ms": timed(lambda: ops.morans_i(F, idx), args.reps)}
        assert torch.equal(idx, ops.spatial_knn(X, K))
        try:
            from sklearn.neighbors import NearestNeighbors
        except ImportError:
            NearestNeighbors = None
        if NearestNeighbors is not None and N <= 200_000:
            Fh = F.cpu().double().numpy()
            t0 = time.perf_counter()
            nb = NearestNeighbors(n_neighbors=K).fit(Xh).kneighbors(return_distance=False)
            t1 = time.perf_counter()
            z = Fh - Fh.mean(0)
            Ih = (z * z[nb].mean(1)).sum(0) / (z * z).sum(0)
            t2 = time.perf_counter()
            r["sklearn_knn_ms"], r["numpy_moran_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
            r["graph_rows_equal_sklearn_sets"] = float(np.mean(np.sort(nb, 1) == np.sort(idx.cpu().numpy(), 1)))
            r["moran_max_abs_diff_numpy"] = float(np.abs(Ih - I.cpu().numpy()).max())
        out["sizes"][str(N)] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
