#!/usr/bin/env python
"""Generate the kmeans_inducing_points golden vectors by running sklearn (build container, CPU only).

    python tests/golden/make_kmeans_golden.py

writes tests/golden/extra_kmeans_<case>.npz -- the ``extra_`` prefix keeps them out of conftest.golden_cases().  Data only.

Per case: X, the start C0, and sklearn's ``KMeans(n_clusters=M, init=C0, n_init=1, algorithm="lloyd", max_iter=...,
tol=...).fit(X)`` (tol = 1e-4 but for the case that is there for a stop by tol): ``centers``, ``labels``, ``inertia``, ``n_iter``; for float32 X also the same run on the float64 cast
of the same values (``centers64`` ...).  A case is written only if (a) the oracle (tests/kmeans_oracle.py) reproduces
sklearn's labels and n_iter_ exactly, (b) over the oracle's whole trajectory every point's best and second-best d^2 differ by
more than 1e-9 relative, (c) for float32 X sklearn's float32 labels equal its float64-cast labels; a draw that fails is
re-seeded (the seed that held is stored).  With each case a seeding fixture: draws ``seed_u`` (M, T) and the oracle's
``seed_idx``, written only if every draw is more than 1e-9 pot from the cumulative-sum entries on either side and every
winning potential beats the runner-up by more than 1e-9 relative.

extra_kmeans_quality.npz: on one data set (N = 2000, M = 64) the final inertia of sklearn's own
``KMeans(init="k-means++", n_init=1, random_state=s)`` and of the oracle (seeding from default_rng(s) + Lloyd) for
s = 0..19, their means and the standard error of the difference of the means."""
import os
import sys
import warnings

import numpy as np
from sklearn.cluster import KMeans

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kmeans_oracle as O  # noqa: E402

GAP = 1e-9
# name: (N, M, d, dtype, max_iter, kind)
CASES = {
    "1037x100_d2_f64": (1037, 100, 2, np.float64, 300, "rows"),
    "1037x100_d2_f32": (1037, 100, 2, np.float32, 300, "rows"),
    "700x65_d3_f64": (700, 65, 3, np.float64, 300, "rows"),
    "300x150_d1_f64": (300, 150, 1, np.float64, 300, "rows"),
    "2051x33_d4_f32": (2051, 33, 4, np.float32, 300, "rows"),
    "40x40_d2_f64": (40, 40, 2, np.float64, 300, "rows"),
    "500x1_d2_f64": (500, 1, 2, np.float64, 300, "rows"),
    "5000x513_d2_f64": (5000, 513, 2, np.float64, 300, "rows"),
    "1037x100_d2_f64_it3": (1037, 100, 2, np.float64, 3, "rows"),
    "600x20_d2_f64_empty": (600, 20, 2, np.float64, 300, "far"),
    "1037x100_d2_f64_tol": (1037, 100, 2, np.float64, 300, "rows"),
}
TOL = {"1037x100_d2_f64_tol": 1e-2}                # every other case: sklearn's default 1e-4
# the stop a case is there for (a draw that stops otherwise is re-seeded); "tol" after more than one iteration
WANT = {"1037x100_d2_f64": "labels", "1037x100_d2_f64_it3": False, "1037x100_d2_f64_tol": "tol", "40x40_d2_f64": "tol"}


def sk(X, C0, max_iter, tol):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = KMeans(n_clusters=len(C0), init=C0.astype(X.dtype), n_init=1, algorithm="lloyd", max_iter=max_iter, tol=tol).fit(X)
    return km.cluster_centers_, km.labels_.astype(np.int32), float(km.inertia_), int(km.n_iter_)


def draw(N, M, d, dtype, kind, rng):
    X = (rng.random((N, d)) * 4 - 2 + 0.3 * rng.normal(size=(N, d))).astype(dtype)
    C0 = X[rng.choice(N, M, replace=False)].astype(np.float64)
    if kind == "far":
        C0[3] = X.max(axis=0).astype(np.float64) + 100.0          # no point is nearest to it: empty on the first iteration
    return X, C0


def make(name):
    N, M, d, dtype, max_iter, kind = CASES[name]
    tol = TOL.get(name, 1e-4)
    for seed in range(1000):
        rng = np.random.default_rng([seed, N, M, d])
        X, C0 = draw(N, M, d, dtype, kind, rng)
        centers, labels, inertia, n_iter = sk(X, C0, max_iter, tol)
        o = O.lloyd(X, C0, max_iter, tol, gap=True)
        if not (np.array_equal(o["labels"], labels) and o["n_iter"] == n_iter and o["min_gap"] > GAP):
            continue
        if name in WANT and (o["converged"] != WANT[name] or (name.endswith("_tol") and n_iter < 2)):
            continue
        out = dict(X=X, C0=C0, centers=centers, labels=labels, inertia=inertia, n_iter=n_iter, max_iter=max_iter, tol=tol, data_seed=seed)
        if dtype == np.float32:
            c64, l64, i64, n64 = sk(X.astype(np.float64), C0, max_iter, tol)
            if not (np.array_equal(l64, labels) and n64 == n_iter):
                continue
            out.update(centers64=c64, labels64=l64, inertia64=i64, n_iter64=n64)
        if kind == "far" and not (o["relocated"] == 1 and len(O.lloyd_iter(X, C0)[3]) == 1):
            continue
        T = O.n_trials(M)
        for s2 in range(1000):
            u = np.random.default_rng([s2, seed, 7]).random((M, T))
            idx, dm, wm = O.seed(X, M, u)
            if dm > GAP and wm > GAP:
                break
        else:
            continue
        out.update(seed_u=u, seed_idx=idx)
        np.savez_compressed(os.path.join(HERE, f"extra_kmeans_{name}.npz"), **out)
        print(f"{name}: data seed {seed}, n_iter {n_iter}, converged {o['converged']}, relocated {o['relocated']}, "
              f"min gap {o['min_gap']:.2e}, seeding margins {dm:.2e} {wm:.2e}", flush=True)
        return
    raise SystemExit(f"{name}: no draw held the conditions")


def quality():
    rng = np.random.default_rng(2024)
    N, M = 2000, 64
    blobs = rng.random((25, 2)) * 4 - 2
    X = blobs[rng.integers(0, 25, N)] + 0.15 * rng.normal(size=(N, 2))
    seeds = np.arange(20)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = np.array([KMeans(n_clusters=M, init="k-means++", n_init=1, algorithm="lloyd", random_state=int(s)).fit(X).inertia_
                      for s in seeds])
    b = np.array([O.kmeans(X, M, random_state=int(s))["inertia"] for s in seeds])
    se = float(np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b)))
    np.savez_compressed(os.path.join(HERE, "extra_kmeans_quality.npz"), X=X, M=M, seeds=seeds, sklearn_inertia=a, oracle_inertia=b,
                        sklearn_mean=a.mean(), oracle_mean=b.mean(), se_diff=se)
    print(f"quality: sklearn {a.mean():.4f}, oracle {b.mean():.4f}, se of the difference {se:.4f}", flush=True)


if __name__ == "__main__":
    for name in CASES:
        make(name)
    quality()
