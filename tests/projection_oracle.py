"""CPU oracle for project_factors_to_inducing (TEST INFRASTRUCTURE ONLY): the kernel least-squares start for gp.mu,
restated in plain torch fp64 with direct-difference distances and the closed forms of the stationary kernels.

    G = K_zx K_xz + jitter I,  b = K_zx f,  alpha = G^-1 b,  mu = K_zz alpha   (whitened: Lz^T alpha, Lz = chol(K_zz + kzz_jitter I))

It is pinned against the notebook's own composition run on the reference's kernels (tests/golden/make_projection_golden.py
-> tests/golden/extra_projection_*.npz; tests/test_projection.py).  The layouts are the library's: G (n, M, M), b (n, R, M)
with n = L, R = 1 for per-latent parameters and n = 1, R = L for scalar ones; alpha and mu are (L, M)."""
from __future__ import annotations

import math

import torch

KINDS = ("rbf", "matern12", "matern32", "matern52")
KIND_CODE = {"rbf": 0, "matern32": 1, "matern12": 4, "matern52": 5}


def kernel_matrix(kind: str, A, B, sigma, lengthscale) -> torch.Tensor:
    """K(A, B) in fp64: (a, b) for 0-d parameters, (L, a, b) for length-L ones."""
    A, B = torch.as_tensor(A).double(), torch.as_tensor(B).double()
    s, ell = torch.as_tensor(sigma).double(), torch.as_tensor(lengthscale).double()
    if s.dim() or ell.dim():
        s, ell = s.reshape(-1, 1, 1), ell.reshape(-1, 1, 1)
    diff = A[:, None, :] - B[None, :, :]
    d2 = (diff * diff).sum(-1)
    if kind == "rbf":
        return s ** 2 * torch.exp(-0.5 * d2 / ell ** 2)
    r = torch.sqrt(d2)
    if kind == "matern12":
        return s ** 2 * torch.exp(-r / ell)
    if kind == "matern32":
        v = math.sqrt(3.0) * r / ell
        return s ** 2 * (1.0 + v) * torch.exp(-v)
    if kind == "matern52":
        v = math.sqrt(5.0) * r / ell
        return s ** 2 * (1.0 + v + v * v / 3.0) * torch.exp(-v)
    raise ValueError(kind)


def project(kind: str, Z, X, F, sigma, lengthscale, jitter: float = 1e-5, kzz_jitter: float = 0.0) -> dict:
    """G, b, alpha, mu (whitened=False), mu_whitened, residual (from the definition: a pass over X), Kzx."""
    F = torch.as_tensor(F).double()
    L = F.shape[0]
    Kzx = kernel_matrix(kind, Z, X, sigma, lengthscale)
    Kzz = kernel_matrix(kind, Z, Z, sigma, lengthscale)
    batched = Kzx.dim() == 3
    M = Kzx.shape[-2]
    eye = torch.eye(M, dtype=torch.float64)
    K3 = Kzx if batched else Kzx[None]
    G = K3 @ K3.transpose(-1, -2) + jitter * eye
    b = (K3 @ F[:, :, None]).transpose(-1, -2) if batched else (F @ Kzx.t())[None]       # (L, 1, M) / (1, L, M)
    a = torch.cholesky_solve(b.transpose(-1, -2), torch.linalg.cholesky(G))              # (n, M, R)
    alpha = a[:, :, 0] if batched else a[0].t()
    Lz = torch.linalg.cholesky(Kzz + kzz_jitter * eye)
    if batched:
        mu = (Kzz @ alpha[:, :, None])[:, :, 0]
        mu_w = (Lz.transpose(-1, -2) @ alpha[:, :, None])[:, :, 0]
        fit = (Kzx.transpose(-1, -2) @ alpha[:, :, None])[:, :, 0]
    else:
        mu, mu_w, fit = alpha @ Kzz, alpha @ Lz, alpha @ Kzx
    residual = ((fit - F) ** 2).sum(1) / (F ** 2).sum(1)
    assert alpha.shape == (L, M)
    return dict(G=G, b=b, alpha=alpha, mu=mu, mu_whitened=mu_w, residual=residual, Kzx=Kzx, Kzz=Kzz)


def svgp_mean(kind: str, Z, X, sigma, lengthscale, mu, jitter: float, whitened: bool) -> torch.Tensor:
    """q(F)'s mean at X of a sparse GP with inducing mean mu (L, M) (reference gp.py:213-228, 270-296): K_xz (K_zz + jitter
    I)^-1 mu, whitened K_xz Lz^-T mu."""
    Kzx = kernel_matrix(kind, Z, X, sigma, lengthscale)
    Kzz = kernel_matrix(kind, Z, Z, sigma, lengthscale)
    M = Kzz.shape[-1]
    Lz = torch.linalg.cholesky(Kzz + jitter * torch.eye(M, dtype=torch.float64))
    mu = torch.as_tensor(mu).double()
    if Kzx.dim() == 2:
        Kzx, Lz = Kzx[None].expand(mu.shape[0], -1, -1), Lz[None].expand(mu.shape[0], -1, -1)
    rhs = mu[:, :, None]
    if whitened:
        v = torch.linalg.solve_triangular(Lz.transpose(-1, -2), rhs, upper=True)
    else:
        v = torch.cholesky_solve(rhs, Lz)
    return (Kzx.transpose(-1, -2) @ v)[:, :, 0]
