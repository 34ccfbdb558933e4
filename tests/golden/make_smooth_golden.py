#!/usr/bin/env python3
"""Generate the smooth_spatial_factors golden vectors by running the REFERENCE and sklearn (build container, CPU only).

    MPLBACKEND=Agg python tests/golden/make_smooth_golden.py

Imports luisdiaz1997/GPzoo from /root/reference like make_nmf_golden.py (read-only, never copied, never shipped) and
writes tests/golden/extra_smooth_<case>.npz -- the ``extra_`` prefix keeps them out of conftest.golden_cases().  Data only.

Per case (N, M, d, L, dtype): spots X uniform in a box, inducing points Z uniform in the same box, factors F = a smooth
field of X plus noise on the log scale, rounded to multiples of 2^-10 (exact in float32; keeps the files small).  Stored:
F, Z, X, K = max(2, ceil(N / M)) and the reference's U, beta0, beta; a float32 case also holds the reference's outputs on
the float64 cast of the same values (U64, beta064, beta64).  A case is only written when
  (a) for every query the K-th and (K+1)-th squared distances differ by more than 1e-5 relative, and
  (b) for float32 cases max|U32 - U64| <= 1e-5 max|U64|
-- the reference's neighbour choice is then unambiguous in both precisions; a draw that fails is re-seeded.

extra_smooth_xnone.npz: the X=None branch (F in float64 and float32).  extra_smooth_helpers.npz: input / output pairs of
rescale_spatial_coords, init_softplus and scanpy_sizefactors.
"""
import os
import sys
from math import ceil

os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, "/root/reference")

import numpy as np

from gpzoo.utilities import (init_softplus, rescale_spatial_coords, scanpy_sizefactors,  # noqa: E402  (the reference)
                             smooth_spatial_factors)

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {
    # name: (N, M, d, L, dtype, collinear)
    "1037x100_d2_L4_f64": (1037, 100, 2, 4, np.float64, False),
    "1037x100_d2_L4_f32": (1037, 100, 2, 4, np.float32, False),
    "300x150_d1_L3_f64": (300, 150, 1, 3, np.float64, False),
    "300x7_d3_L5_f64": (300, 7, 3, 5, np.float64, False),
    "4099x33_d4_L64_f32": (4099, 33, 4, 64, np.float32, False),
    "40x64_d2_L3_f64": (40, 64, 2, 3, np.float64, False),
    "collinear_500x40_d2_L3_f64": (500, 40, 2, 3, np.float64, True),
}


def draw(N, M, d, L, dtype, collinear, seed):
    rng = np.random.default_rng(seed)
    if collinear:
        X = rng.random((N, 1)) * 4.0 * np.array([[1.0, 0.5]]) + np.array([[-2.0, -0.7]])
        Z = rng.random((M, 1)) * 4.0 * np.array([[1.0, 0.5]]) + np.array([[-2.0, -0.7]])
    else:
        X, Z = rng.random((N, d)) * 4.0 - 2.0, rng.random((M, d)) * 4.0 - 2.0
    F = np.sin(X @ rng.normal(size=(d, L))) + 0.3 * rng.normal(size=(N, L)) - 1.5
    F = np.round(F * 1024.0) / 1024.0
    return F.astype(dtype), Z.astype(dtype), X.astype(dtype)


def kth_gap(X, Z, K):
    """min over the queries of (d2[K] - d2[K-1]) / d2[K] for the sorted squared distances (fp64, separately rounded)."""
    X, Z = X.astype(np.float64), Z.astype(np.float64)
    d2 = (X[None, :, 0] - Z[:, None, 0]) ** 2
    for k in range(1, X.shape[1]):
        d2 = d2 + (X[None, :, k] - Z[:, None, k]) ** 2
    d2.sort(axis=1)
    return ((d2[:, K] - d2[:, K - 1]) / d2[:, K]).min()


def main():
    for name, (N, M, d, L, dtype, collinear) in CASES.items():
        K = max(2, ceil(N / M))
        for seed in range(100, 200):
            F, Z, X = draw(N, M, d, L, dtype, collinear, seed)
            gap = kth_gap(X, Z, K)
            if not gap > 1e-5:
                print(f"{name}: seed {seed} fails (a), gap {gap:.1e}")
                continue
            U, beta0, beta = smooth_spatial_factors(F.copy(), Z.copy(), X.copy())
            out = dict(F=F, Z=Z, X=X, K=K, U=U, beta0=beta0, beta=beta)
            if dtype is np.float32:
                U64, b064, b64 = smooth_spatial_factors(F.astype(np.float64), Z.astype(np.float64), X.astype(np.float64))
                dev = np.abs(U - U64).max() / np.abs(U64).max()
                if not dev <= 1e-5:
                    print(f"{name}: seed {seed} fails (b), {dev:.1e}")
                    continue
                out.update(U64=U64, beta064=b064, beta64=b64)
            break
        else:
            raise SystemExit(f"{name}: no seed meets (a) and (b)")
        path = os.path.join(HERE, f"extra_smooth_{name}.npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 1000 * 1000, os.path.getsize(path)
        print(f"{name}: seed {seed}, K {K}, gap {gap:.1e}, U {U.dtype}, beta0 {beta0.dtype}, beta {beta.dtype}, "
              f"{os.path.getsize(path)} bytes")

    rng = np.random.default_rng(7)
    F = np.round((rng.normal(size=(211, 6)) - 1.5) * 1024.0) / 1024.0
    Z = rng.random((9, 2))
    out = dict(F=F, Z=Z)
    for tag, dt in (("64", np.float64), ("32", np.float32)):
        U, beta0, beta = smooth_spatial_factors(F.astype(dt), Z)
        assert beta is None
        out["U" + tag], out["beta0" + tag] = U, beta0
    np.savez_compressed(os.path.join(HERE, "extra_smooth_xnone.npz"), **out)

    out = {}
    coords = rng.random((157, 2)) * np.array([[6400.0, 3100.0]]) + np.array([[1200.0, 800.0]])
    for tag, dt in (("64", np.float64), ("32", np.float32)):
        out["coords" + tag] = coords.astype(dt)
        out["rescaled" + tag] = rescale_spatial_coords(coords.astype(dt))           # (the reference works in place: a copy)
        out["rescaled6_" + tag] = rescale_spatial_coords(coords.astype(dt), box_side=6)
        mat = (rng.random((40, 5)) * 30.0 + 1e-3).astype(dt)                            # both sides of the threshold 20
        out["mat" + tag] = mat
        out["softplus" + tag] = init_softplus(mat)
        out["softplus_min" + tag] = init_softplus(mat, minval=1e-3)
        counts = rng.poisson(3.0, size=(60, 25)).astype(dt)
        out["counts" + tag] = counts
        out["sizefactors" + tag] = scanpy_sizefactors(counts)
    out["coords3d"] = rng.random((80, 3)) * np.array([[10.0, 20.0, 5.0]])
    out["rescaled3d"] = rescale_spatial_coords(out["coords3d"].copy())
    np.savez_compressed(os.path.join(HERE, "extra_smooth_helpers.npz"), **out)
    print("xnone, helpers written")


if __name__ == "__main__":
    main()
