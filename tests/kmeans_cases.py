"""Shapes and data builders of tests/test_hip_kmeans.py and the reason for each (TEST INFRASTRUCTURE ONLY; numpy,
importable without a GPU -- tests/test_kmeans_cases.py checks everything here on the CPU, including that the constants
below are the ``constexpr`` values of gpzoo_amd/csrc/kmeans.hip: a retune cannot move the edges off the tests).

    T_C         centres per LDS tile of the assignment: a centre count of T_C - 1 / T_C / T_C + 1 / 2 T_C + 1 ends a tile one
                short, exactly, one over, and makes a third tile of one centre
    B_N         points per workgroup (one per lane), and per block total of the seeding's cumulative sum and the inertia
    S           member stride of the cluster sums: lane j of a cluster's wave adds the members among the points j (mod S)
    SPLIT_WGS   with fewer point tiles than this the centre tiles are split over several workgroups per point tile
"""
from __future__ import annotations

import numpy as np

T_C, B_N, S, SPLIT_WGS = 256, 256, 64, 1024
GOLDENS = ["1037x100_d2_f64", "1037x100_d2_f32", "700x65_d3_f64", "300x150_d1_f64", "2051x33_d4_f32", "40x40_d2_f64",
           "500x1_d2_f64", "5000x513_d2_f64", "1037x100_d2_f64_it3", "600x20_d2_f64_empty", "1037x100_d2_f64_tol"]
# what a golden is there for: its stop, and whether its first iteration relocates
GOLDEN_STOP = {"1037x100_d2_f64": "labels", "1037x100_d2_f64_it3": False, "1037x100_d2_f64_tol": "tol", "40x40_d2_f64": "tol"}


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def split_plan(N: int, M: int) -> dict:
    """kms_split (csrc/kmeans.hip): workgroups per point tile and centre tiles each of them takes."""
    tiles, ctiles = cdiv(N, B_N), cdiv(M, T_C)
    want = 1 if tiles >= SPLIT_WGS else cdiv(SPLIT_WGS, tiles)
    want = min(want, ctiles)
    tps = cdiv(ctiles, want)
    return dict(tiles=tiles, ctiles=ctiles, tiles_per_split=tps, splits=cdiv(ctiles, tps))


EDGE_M = [1, T_C - 1, T_C, T_C + 1, 2 * T_C + 1]


def edge_n(M: int) -> list:
    return sorted({n for n in (M, B_N - 1, B_N, B_N + 1, 2 * B_N + 3) if n >= M})


def edge_cases() -> list:
    """(N, M, d, dtype name): every (M, N) edge pair with d and the dtype cycling, then every (d, dtype) at one shape
    with a ragged last centre tile, a ragged last point tile and two centre splits."""
    out, i = [], 0
    for M in EDGE_M:
        for N in edge_n(M):
            out.append((N, M, 1 + i % 4, ("f64", "f32")[(i // 4) % 2]))
            i += 1
    out += [(2 * B_N + 3, T_C + 1, d, t) for d in (1, 2, 3, 4) for t in ("f64", "f32")]
    return out


# the assignment's two paths, each on both sides of its switches: (N, M, what)
PATH_CASES = [
    (2 * T_C + 3, T_C, "one centre tile: one workgroup per point tile"),
    (2 * T_C + 3, T_C + 1, "two centre tiles: split in two"),
    (2 * T_C + 3, 2 * T_C + 1, "three centre tiles: split in three"),
    ((SPLIT_WGS // 2) * B_N, 2 * T_C + 1, "SPLIT_WGS / 2 point tiles: two splits of two and one centre tiles"),
    ((SPLIT_WGS - 1) * B_N, T_C + 1, "one point tile short of SPLIT_WGS: still split"),
    ((SPLIT_WGS - 1) * B_N + 1, T_C + 1, "SPLIT_WGS point tiles: one workgroup per point tile walks both centre tiles"),
]

BLOB_SIZES = [1, S - 1, S, S + 1, 2 * S + 1]


def dtype_of(name: str):
    return np.float32 if name == "f32" else np.float64


def random_case(N: int, M: int, d: int, dtype="f64", seed: int = 0):
    """X (N,d) of the dtype and a start C0 (M,d) fp64: M distinct rows of X pushed a little off the points."""
    rng = np.random.default_rng([seed, N, M, d])
    X = (rng.random((N, d)) * 4 - 2).astype(dtype_of(dtype))
    C0 = X[rng.choice(N, M, replace=False)].astype(np.float64) + 0.05 * rng.normal(size=(M, d))
    return X, C0


def blob_case(sizes=BLOB_SIZES, d: int = 2, seed: int = 1):
    """Tight blobs of the given sizes around centres 10 apart, the points shuffled: X, C0 = the blob centres, and the size
    of each cluster (a start centre's cluster is its blob)."""
    rng = np.random.default_rng(seed)
    centres = np.zeros((len(sizes), d))
    centres[:, 0] = 10.0 * np.arange(len(sizes))
    X = np.concatenate([c + 0.1 * rng.normal(size=(s, d)) for c, s in zip(centres, sizes)])
    X = X[rng.permutation(len(X))]
    return X, centres, list(sizes)


def tie_case():
    """Ten copies of the origin and ten of (0, 4) between centres at equal distances: centre 3 = (-1, 0) and centre T_C + 43
    = (1, 0) (another LDS tile, another split) tie for the origin; centres 5 and 9 are both (0, 5), so 9 is left empty.
    The other centres are far away with one point each."""
    M = T_C + 44
    C0 = np.zeros((M, 2))
    C0[:, 0] = 100.0 + 3.0 * np.arange(M)
    C0[3], C0[M - 1], C0[5], C0[9] = (-1.0, 0.0), (1.0, 0.0), (0.0, 5.0), (0.0, 5.0)
    own = np.array([m for m in range(M) if m not in (3, M - 1, 5, 9)])
    X = np.concatenate([np.zeros((10, 2)), np.tile([[0.0, 4.0]], (10, 1)), C0[own] + 0.25])
    return X, C0


def empty_case(n_empty: int, N: int = 700, M: int = 12, seed: int = 3):
    """Random points and a start whose last n_empty centres lie far outside the data: empty on the first iteration."""
    X, C0 = random_case(N, M, 2, "f64", seed)
    C0[M - n_empty:] = 50.0 + 10.0 * np.arange(n_empty)[:, None]
    return X, C0


def few_distinct_case():
    """N = 40 points of which 10 are distinct, M = 16 (a draw on which no two candidates of the seeding at different
    positions have potentials within rounding of each other: tests/test_kmeans_cases.py)."""
    rng = np.random.default_rng(9)
    base = rng.random((10, 2)) * 4 - 2
    return base[np.arange(40) % 10].copy(), 16
