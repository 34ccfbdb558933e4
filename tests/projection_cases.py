"""Shapes and data builders of tests/test_hip_projection.py and the reason for each (TEST INFRASTRUCTURE ONLY; numpy,
importable without a GPU -- tests/test_projection_cases.py checks everything here on the CPU).  The tile size, the column
step and the N-splits are not restated here: they are read from ``gpz_kernel_gram_plan``, a host-only query of the
library, so a retune of csrc/gram.hip moves the edge cases with it.

A case: ``name``, ``kind`` (projection_oracle.KINDS), ``d``, ``dtype`` ("f32" / "f64"), ``per_latent`` (per-latent
parameters: n = L Gram matrices with R = 1 right-hand side each; else one Gram matrix with R = L), ``L``, ``M``, ``N`` (a
number, or ("step", k) = the column step of the precision + k) and ``why``."""
from __future__ import annotations

import math

import numpy as np

# reference-generated fixtures (tests/golden/make_projection_golden.py): name -> (N, M, L, frac, reference kernel class,
# per-latent parameters)
GOLDENS = {
    "300x40_L3_rbf": (300, 40, 3, 0.5, "RBF", False),
    "1037x130_L4_nsf_rbf": (1037, 130, 4, 0.5, "NSF_RBF", True),
    "2100x257_L2_batched_matern32": (2100, 257, 2, 0.5, "batched_Matern32", True),
    "700x129_L3_batched_rbf": (700, 129, 3, 0.6, "batched_RBF", True),
    "4200x385_L2_matern32_scalar": (4200, 385, 2, 0.5, "batched_Matern32", False),
}
GOLDEN_KIND = {"RBF": "rbf", "NSF_RBF": "rbf", "batched_RBF": "rbf", "batched_Matern32": "matern32"}
COND_MAX, REF32_ERR_MAX = 1e4, 1e-4       # what a fixture has to hold to be used for a value comparison

EDGE_M = (1, 127, 128, 129, 257)
EDGE_N = (1, ("step", -1), ("step", 0), ("step", 1))


def recipe(N: int, M: int, L: int, frac: float, seed, d: int = 2, per_latent: bool = True) -> dict:
    """The well-conditioned inputs every comparison of mu uses: X uniform in [-2, 2]^d; Z a random subset of a g^d grid of
    cell centres over the box (g = ceil(M^(1/d)), pitch 4 / g), each point displaced by up to +-0.15 pitch per coordinate;
    lengthscale_l = frac pitch (1 + 0.1 l), sigma_l = 1 + 0.1 l (l = 0 alone for scalar parameters);
    F_l = sin((l + 1) x_0) + 0.1 noise.  Everything is rounded to float32 and returned as float32, so the fp32 and the fp64
    path (which gets the float64 cast) see the same numbers.  (Inducing points drawn from the spots themselves with a
    lengthscale near their spacing give cond(G) >= 1e8: no value comparison may use such inputs.)"""
    rng = np.random.default_rng([int(s) for s in np.atleast_1d(seed)] + [N, M, L, d])
    X = rng.random((N, d)) * 4 - 2
    g = 1
    while g ** d < M:
        g += 1
    pitch = 4.0 / g
    cells = rng.choice(g ** d, M, replace=False)
    idx = np.stack(np.unravel_index(cells, (g,) * d), axis=1)
    Z = -2 + (idx + 0.5) * pitch + (rng.random((M, d)) * 2 - 1) * 0.15 * pitch
    l = np.arange(L if per_latent else 1)
    ell, sigma = frac * pitch * (1 + 0.1 * l), 1 + 0.1 * l
    F = np.sin((np.arange(L)[:, None] + 1) * X[None, :, 0]) + 0.1 * rng.normal(size=(L, N))
    if not per_latent:
        ell, sigma = ell[0], sigma[0]
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    return dict(X=f32(X), Z=f32(Z), F=f32(F), sigma=f32(sigma), lengthscale=f32(ell), pitch=pitch)


def _case(name, kind, d, dtype, per_latent, L, M, N, why):
    return dict(name=name, kind=kind, d=d, dtype=dtype, per_latent=per_latent, L=L, M=M, N=N, why=why)


def cases() -> list:
    from projection_oracle import KINDS
    out = []
    # every kernel instance -- (kind, precision, right-hand-side block: R <= 16 / R > 16) -- with M, N and d cycling
    # through their edges
    i = 0
    for kind in KINDS:
        for dtype in ("f32", "f64"):
            for per_latent, L in ((True, 2), (False, 20)):
                M, N, d = EDGE_M[i % 5], (EDGE_N + (300, 1037))[i % 6], 1 + i % 4
                out.append(_case(f"inst{i}_{kind}_{dtype}_{'lat' if per_latent else 'sc'}", kind, d, dtype, per_latent, L, M, N,
                                 "one kernel instance; M, N, d cycle through their edges"))
                i += 1
    # every edge of M against every edge of N, both precisions (the column step differs)
    for dtype in ("f32", "f64"):
        for M in EDGE_M:
            for N in EDGE_N:
                out.append(_case(f"edge_M{M}_N{N if isinstance(N, int) else 'step%+d' % N[1]}_{dtype}", "rbf", 2, dtype, True, 2, M, N,
                                 "tile edge x column-step edge"))
    out += [
        _case("splits_f32", "rbf", 2, "f32", False, 3, 40, 300, ">= 3 N-splits, the last one short and ending inside a step"),
        _case("splits_f64", "matern32", 2, "f64", True, 3, 40, 300, "the same in fp64"),
        _case("far_tile_f32", "matern52", 3, "f32", True, 2, 257, 1037,
              "three row tiles: tile (2, 0) touches no diagonal tile; many short splits"),
        _case("far_tile_f64", "matern12", 4, "f64", False, 4, 257, 700, "the same in fp64, scalar parameters, R = 4"),
        _case("r16_f32", "rbf", 2, "f32", False, 16, 130, 200, "R = 16: the last size of the small right-hand-side block"),
        _case("r17_f32", "rbf", 2, "f32", False, 17, 130, 200, "R = 17: the first size of the large one"),
        _case("r64_f64", "rbf", 1, "f64", False, 64, 129, 100, "R = 64: the limit"),
        _case("one_latent_f32", "matern32", 2, "f32", True, 1, 33, 77, "L = 1 with per-latent parameters: R = 1, n = 1"),
    ]
    return out


def plan_of(case) -> dict:
    """The library's plan of a case (host-only query).  N is resolved first: a ("step", k) needs the precision's step."""
    import torch
    from gpzoo_amd import ops
    dt = torch.float32 if case["dtype"] == "f32" else torch.float64
    n = case["L"] if case["per_latent"] else 1
    N = case["N"]
    if not isinstance(N, int):
        N = ops.kernel_gram_plan(1, case["M"], n, dt)["col_step"] + N[1]
    p = ops.kernel_gram_plan(N, case["M"], n, dt)
    p["N"] = N
    return p


def data_of(case, N: int) -> dict:
    """Inputs of a case by the recipe (frac 0.8: neighbouring inducing points overlap, entries of every size)."""
    return recipe(N, case["M"], case["L"], 0.8, [7, len(case["name"])], d=case["d"], per_latent=case["per_latent"])


def np_dtype(name: str):
    return np.float32 if name == "f32" else np.float64


def cdiv(a: int, b: int) -> int:
    return math.ceil(a / b)
